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
//   k_ip_gather   a workgroup per block copies u32 payload_bytes, head, table and strands -- or the stored text -- to their byte-granular place: whole dwords
//                 of the destination inside the block, the bytes in front of and behind them one by one.  Nothing outside the blocks is written.
// A lane's walk over its own lines is byte-serial and not coalesced: neighbouring lanes read text q lines apart.  That is accepted here (NOTES.md has the rate).
//
// Unpacking.  The block offsets follow from the payload_bytes prefixes and the places in the text from the block_text_bytes behind them (k_ip_walk, one lane;
// the file call walks them on the host with pread).
//   k_ip_decode   a workgroup per block validates head, bitmap, rows and strand sizes into LDS (id_check_head, id_load_row, id_check_strand), then a lane per
//                 strand decodes forward (id_strand_decode) and writes its text at its prefix-summed offset.  Any violation raises the error word:
//                 block number << 8 | ID_E_*.
#include "devutil.h"
#include "id_block.h"
#include "fileio.h"

#define IP_T 256
#define IP_HDR ((ID_HEAD1 + 2u * ID_TABLE + 15u) & ~15u)          // the head and table of a coded payload, rounded to 16
#define IP_CALL_TEXT ((uint64_t)256 << 20)                        // the file call: text of one kernel call, where more than one block would be more (HARC_AMD_IDPACK_CALL_TEXT in tests)

struct IpShared {
    uint32_t fc[ID_TABLE];
    uint32_t bm[4], present[ID_ROWS], bad, err, verr, mode, tbytes, hdr1, newlines;
    uint32_t scan[IP_T / 64 + 1];
    unsigned long long tsum, lsum;
};
struct IpGather { uint32_t scan[IP_T / 64 + 1], soff[ID_STRANDS], slen[ID_STRANDS]; };
struct IpStats { uint64_t text = 0, bytes = 0, blocks = 0, stored = 0; double seconds = 0; };

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
    __shared__ IpGather S;
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
    const uint8_t *hdr = heads + b * (uint64_t)IP_HDR;
    const uint32_t len = qv_le32(hdr + ID_HEAD0 + 4u * ID_STRANDS + 4u * t);
    uint32_t total;
    const uint32_t off = block_excl_scan_u32<IP_T>(len, S.scan, &total);
    const uint32_t h = payload - total;
    S.soff[t] = off; S.slen[t] = len;
    group_copy_bytes(dst + 4, hdr, h, t, IP_T);
    __syncthreads();
    const uint32_t wv = t >> 6, lane = t & 63u;
    for (uint32_t s = wv; s < ID_STRANDS; s += IP_T / 64) {
        const uint32_t n = S.slen[s];
        if (n) group_copy_bytes(dst + 4 + h + S.soff[s], slabs + sat[(uint64_t)ID_STRANDS * b + s], n, lane, 64);
    }
}

// The offsets of the nb blocks behind the 32-byte header of p[0 .. n_bytes), relative to p + 32, and of their text; off[nb] / toff[nb] = their ends.
// bad[0]: 1 + the first block whose prefix, head or payload leaves the bytes or whose text is longer than 2^30 bytes (nb + 1: bytes are left behind the last block,
// nb + 2: the text bytes of the blocks are not those of the header), bad[1]: its offset
__global__ void k_ip_walk(const uint8_t *p, uint64_t n_bytes, uint64_t nb, uint64_t text_bytes, uint64_t *off, uint64_t *toff, unsigned long long *bad)
{
    if (threadIdx.x || blockIdx.x) return;
    uint64_t at = ID_FILE_HEADER, tat = 0;
    for (uint64_t b = 0; b < nb; b++) {
        off[b] = at - ID_FILE_HEADER; toff[b] = tat;
        if (n_bytes - at < 4u + ID_HEAD0) { bad[0] = b + 1; bad[1] = at; return; }
        const uint64_t pb = qv_le32(p + at), tb = qv_le32(p + at + 5);
        if (pb < ID_HEAD0 || n_bytes - at - 4 < pb || tb > ID_MAX_BLOCK_TEXT || tb > text_bytes - tat) { bad[0] = b + 1; bad[1] = at; return; }
        at += 4 + pb; tat += tb;
    }
    off[nb] = at - ID_FILE_HEADER; toff[nb] = tat;
    if (at != n_bytes) { bad[0] = nb + 1; bad[1] = at; }
    else if (tat != text_bytes) { bad[0] = nb + 2; bad[1] = tat; }
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
                           uint64_t *n_out, uint64_t block0, IpStats *st)
{
    *n_out = 0;
    const uint64_t nb64 = id_blocks(n, RB);
    if (nb64 > 0x7FFFFFF0ull / ID_STRANDS) { harc_set_error("idpack: too many blocks for one call"); return HARC_AMD_EINVAL; }
    const uint32_t nb = (uint32_t)nb64;
    if (!nb) return HARC_AMD_OK;
    PoolScope scope(c);
    const uint64_t nev = (t1 - t0) + 2ull * n;
    uint16_t *events = nullptr; uint8_t *slabs = nullptr, *heads = nullptr; uint64_t *sat = nullptr, *btext = nullptr, *boff = nullptr; uint32_t *bsize = nullptr, *bmode = nullptr;
    unsigned int *d_err = nullptr;
    RC_TRY(dalloc(c, &events, (size_t)nev)); RC_TRY(dalloc(c, &slabs, (size_t)(2ull * nev + 32ull * ID_STRANDS * nb))); RC_TRY(dalloc(c, &heads, (size_t)IP_HDR * nb));
    RC_TRY(dalloc(c, &sat, (size_t)ID_STRANDS * nb)); RC_TRY(dalloc(c, &btext, (size_t)nb)); RC_TRY(dalloc(c, &boff, (size_t)nb + 1));
    RC_TRY(dalloc(c, &bsize, (size_t)nb + 1)); RC_TRY(dalloc(c, &bmode, (size_t)nb)); RC_TRY(dalloc(c, &d_err, 4));
    HIP_TRY(hipMemsetAsync(bsize + nb, 0, 4, c->stream));
    HIP_TRY(hipMemsetAsync(d_err, 0, 16, c->stream));
    HIP_TRY(hipMemsetAsync(d_err, 0xFF, 4, c->stream));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct EvGuard { hipEvent_t &a, &b; ~EvGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } evguard{ e0, e1 };
    if (st) { HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1)); HIP_TRY(hipEventRecord(e0, c->stream)); }
    hipLaunchKernelGGL(k_ip_encode, harc_fold256(nb), dim3(IP_T), 0, c->stream, (const uint8_t *)d_text, nls, t0, n, RB, nb, events, slabs, heads, sat, btext, bsize, bmode, d_err);
    HIP_TRY(hipGetLastError());
    RC_TRY(prim_excl_scan_u32_to_u64(c, bsize, boff, (size_t)nb + 1));
    uint64_t total = 0; unsigned int err[4] = { 0, 0, 0, 0 };
    HIP_TRY(hipMemcpyAsync(&total, boff + nb, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(err, d_err, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (err[0] != 0xFFFFFFFFu) { harc_set_error("idpack: the text of block %llu is longer than %u bytes", (unsigned long long)(block0 + err[0] - 1), ID_MAX_BLOCK_TEXT); return HARC_AMD_EINVAL; }
    if (err[1]) { harc_set_error("idpack: %u strands did not fit their scratch", err[1]); return HARC_AMD_EINTERNAL; }
    *n_out = total;
    if (st) { st->text += t1 - t0; st->bytes += total; st->blocks += nb; st->stored += err[2]; }
    if (d_out) {
        if (out_capacity < total) { harc_set_error("idpack_device: the blocks take %llu bytes, the buffer holds %llu", (unsigned long long)total, (unsigned long long)out_capacity); return HARC_AMD_EINVAL; }
        hipLaunchKernelGGL(k_ip_gather, harc_fold256(nb), dim3(IP_T), 0, c->stream, (const uint8_t *)d_text, nb, (const uint8_t *)slabs, (const uint8_t *)heads, (const uint64_t *)sat,
                           (const uint64_t *)btext, (const uint32_t *)bsize, (const uint32_t *)bmode, (const uint64_t *)boff, d_out);
        HIP_TRY(hipGetLastError());
    }
    if (st) {
        HIP_TRY(hipEventRecord(e1, c->stream)); HIP_TRY(hipEventSynchronize(e1));
        float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1); st->seconds += 1e-3 * (double)ms;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));                     // the scratch goes back to the pool
    return HARC_AMD_OK;
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
    if (!c || (text_bytes && !d_text) || !n_out) { harc_set_error("idpack_device: bad arguments"); return HARC_AMD_EINVAL; }
    const uint32_t rb = ip_rb(lines_per_block);
    HIP_TRY(hipSetDevice(c->P.device));
    const uint64_t head = (flags & HARC_AMD_IDPACK_NO_HEADER) ? 0 : ID_FILE_HEADER;
    const bool trace = getenv("HARC_AMD_TRACE") != nullptr;
    IpStats st; uint64_t nblk = 0, n = 0;
    *n_out = head;
    // the size first: a buffer that is too small is refused with both numbers before a byte of it is written
    if (d_out && out_capacity < head) { harc_set_error("idpack_device: the blocks take at least %llu bytes, the buffer holds %llu", (unsigned long long)head, (unsigned long long)out_capacity); return HARC_AMD_EINVAL; }
    PoolScope scope(c);
    if (text_bytes) {
        const uint64_t *nls = nullptr;
        RC_TRY(ip_index(c, "idpack_device", d_text, text_bytes, &nls, &n));
        const int rc = harc_idpack_run(c, d_text, nls, 0, text_bytes, n, rb, d_out ? d_out + head : nullptr, d_out ? out_capacity - head : 0, &nblk, 0, trace ? &st : nullptr);
        *n_out = head + nblk;
        if (rc != HARC_AMD_OK) {
            if (d_out && nblk && out_capacity - head < nblk) harc_set_error("idpack_device: the packed form takes %llu bytes, the buffer holds %llu", (unsigned long long)(head + nblk), (unsigned long long)out_capacity);
            return rc;
        }
    }
    if (d_out && head) {
        uint8_t h[ID_FILE_HEADER];
        id_file_header(h, rb, n, text_bytes);
        HIP_TRY(hipMemcpyAsync(d_out, h, ID_FILE_HEADER, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (trace) fprintf(stderr, "[idpack] device call: %llu bytes of text -> %llu bytes in %llu blocks (%llu stored), kernels %.3f ms (%.2f GB/s of text)\n", (unsigned long long)text_bytes,
                       (unsigned long long)*n_out, (unsigned long long)st.blocks, (unsigned long long)st.stored, 1e3 * st.seconds, st.seconds > 0 ? 1e-9 * (double)st.text / st.seconds : 0.0);
    return HARC_AMD_OK;
}

// ------------------------------------------------------------------------------------------------ unpacking
struct IdHeader { uint32_t rb; uint64_t n, text, nb; };
// the 32 bytes at h of a packed form of n_bytes bytes
static int ip_parse_header(const char *who, const uint8_t *h, uint64_t n_bytes, IdHeader *H)
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
// nb blocks at d_blocks with their offsets d_off[0 .. nb] and text offsets d_toff[0 .. nb] -> the n lines at d_text; block0 / base: number and file offset of the
// first of them, for the message
static int harc_idunpack_run(harc_amd_ctx *c, const uint8_t *d_blocks, const uint64_t *d_off, const uint64_t *d_toff, const uint64_t *h_off, uint32_t nb, uint64_t n, uint32_t RB,
                             char *d_text, uint64_t block0, uint64_t base)
{
    if (!nb) return HARC_AMD_OK;
    PoolScope scope(c);
    unsigned long long *d_errw = nullptr; RC_TRY(dalloc(c, &d_errw, 2));
    HIP_TRY(hipMemsetAsync(d_errw, 0xFF, 8, c->stream));
    hipLaunchKernelGGL(k_ip_decode, harc_fold256(nb), dim3(IP_T), 0, c->stream, d_blocks, d_off, d_toff, nb, n, RB, (uint8_t *)d_text, d_errw);
    HIP_TRY(hipGetLastError());
    unsigned long long errw = 0;
    HIP_TRY(hipMemcpyAsync(&errw, d_errw, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (errw != ~0ull) {
        const uint64_t b = errw >> 8;
        harc_set_error("idunpack: block %llu at byte %llu is damaged: %s", (unsigned long long)(block0 + b), (unsigned long long)(base + (h_off ? h_off[b] : 0)), id_error_text((uint32_t)(errw & 0xFF)));
        return HARC_AMD_EINVAL;
    }
    return HARC_AMD_OK;
}

extern "C" int harc_amd_idunpack_device(harc_amd_ctx *c, const uint8_t *d_packed, uint64_t n_bytes, char *d_text, uint64_t out_capacity, uint64_t *n_out)
{
    if (!c || !d_packed || !n_out) { harc_set_error("idunpack_device: bad arguments"); return HARC_AMD_EINVAL; }
    if (n_bytes < ID_FILE_HEADER) { harc_set_error("idunpack_device: %llu bytes are fewer than the %u of the header", (unsigned long long)n_bytes, ID_FILE_HEADER); return HARC_AMD_EINVAL; }
    HIP_TRY(hipSetDevice(c->P.device));
    uint8_t h[ID_FILE_HEADER];
    HIP_TRY(hipMemcpyAsync(h, d_packed, ID_FILE_HEADER, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    IdHeader H;
    RC_TRY(ip_parse_header("idunpack_device", h, n_bytes, &H));
    *n_out = H.text;
    if (!d_text) return HARC_AMD_OK;
    if (out_capacity < H.text) { harc_set_error("idunpack_device: the text takes %llu bytes, the buffer holds %llu", (unsigned long long)H.text, (unsigned long long)out_capacity); return HARC_AMD_EINVAL; }
    if (!H.nb) return HARC_AMD_OK;
    if (H.nb > 0x7FFFFFF0ull) { harc_set_error("idunpack_device: too many blocks for one call"); return HARC_AMD_EINVAL; }
    PoolScope scope(c);
    uint64_t *d_off = nullptr, *d_toff = nullptr; unsigned long long *d_bad = nullptr;
    RC_TRY(dalloc(c, &d_off, (size_t)H.nb + 1)); RC_TRY(dalloc(c, &d_toff, (size_t)H.nb + 1)); RC_TRY(dalloc(c, &d_bad, 2));
    HIP_TRY(hipMemsetAsync(d_bad, 0, 16, c->stream));
    hipLaunchKernelGGL(k_ip_walk, dim3(1), dim3(64), 0, c->stream, d_packed, n_bytes, H.nb, H.text, d_off, d_toff, d_bad);
    HIP_TRY(hipGetLastError());
    unsigned long long bad[2] = { 0, 0 };
    std::vector<uint64_t> h_off((size_t)H.nb + 1);
    HIP_TRY(hipMemcpyAsync(bad, d_bad, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (bad[0]) {
        if (bad[0] == H.nb + 2) harc_set_error("idunpack_device: block %llu ends the text at byte %llu, the header announces %llu", (unsigned long long)H.nb - 1, bad[1], (unsigned long long)H.text);
        else if (bad[0] == H.nb + 1) harc_set_error("idunpack_device: block %llu ends at byte %llu, but there are %llu bytes", (unsigned long long)H.nb - 1, bad[1], (unsigned long long)n_bytes);
        else harc_set_error("idunpack_device: block %llu at byte %llu leaves the %llu bytes of the packed form or the %llu bytes of its text", bad[0] - 1, bad[1], (unsigned long long)n_bytes, (unsigned long long)H.text);
        return HARC_AMD_EINVAL;
    }
    HIP_TRY(hipMemcpyAsync(h_off.data(), d_off, 8 * ((size_t)H.nb + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return harc_idunpack_run(c, d_packed + ID_FILE_HEADER, d_off, d_toff, h_off.data(), (uint32_t)H.nb, H.n, H.rb, d_text, 0, ID_FILE_HEADER);
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

// the u32 and the head of block b at byte `at` of a packed form of n_bytes bytes, read into q[9]: its payload and text bytes, checked against what is left
static int ip_check_prefix(const char *who, const uint8_t *q, uint64_t b, uint64_t at, uint64_t n_bytes, uint64_t text_left, uint64_t *pb, uint64_t *tb)
{
    *pb = qv_le32(q); *tb = qv_le32(q + 5);
    if (*pb < ID_HEAD0 || n_bytes - at - 4 < *pb || *tb > ID_MAX_BLOCK_TEXT || *tb > text_left) {
        harc_set_error("%s: block %llu at byte %llu leaves the %llu bytes of the packed form or the bytes of its text", who, (unsigned long long)b, (unsigned long long)at, (unsigned long long)n_bytes);
        return HARC_AMD_EINVAL;
    }
    return HARC_AMD_OK;
}

extern "C" int harc_amd_idunpack_host(const uint8_t *packed, uint64_t n_bytes, char *text, uint64_t cap, uint64_t *n_out)
{
    if (!packed || !n_out) { harc_set_error("idunpack_host: bad arguments"); return HARC_AMD_EINVAL; }
    if (n_bytes < ID_FILE_HEADER) { harc_set_error("idunpack_host: %llu bytes are fewer than the %u of the header", (unsigned long long)n_bytes, ID_FILE_HEADER); return HARC_AMD_EINVAL; }
    IdHeader H;
    RC_TRY(ip_parse_header("idunpack_host", packed, n_bytes, &H));
    *n_out = H.text;
    if (!text) return HARC_AMD_OK;
    if (cap < H.text) { harc_set_error("idunpack_host: the text takes %llu bytes, the buffer holds %llu", (unsigned long long)H.text, (unsigned long long)cap); return HARC_AMD_EINVAL; }
    std::vector<IdWork> W(1);
    uint64_t at = ID_FILE_HEADER, tat = 0;
    for (uint64_t b = 0; b < H.nb; b++) {
        if (n_bytes - at < 4u + ID_HEAD0) { harc_set_error("idunpack_host: block %llu at byte %llu leaves the %llu bytes of the packed form", (unsigned long long)b, (unsigned long long)at, (unsigned long long)n_bytes); return HARC_AMD_EINVAL; }
        uint64_t pb = 0, tb = 0;
        RC_TRY(ip_check_prefix("idunpack_host", packed + at, b, at, n_bytes, H.text - tat, &pb, &tb));
        const uint64_t line0 = b * (uint64_t)H.rb;
        const uint32_t m = H.n - line0 < H.rb ? (uint32_t)(H.n - line0) : H.rb;
        const int e = id_block_decode(packed + at + 4, (uint32_t)pb, m, W[0], (uint8_t *)text + tat);
        if (e) { harc_set_error("idunpack: block %llu at byte %llu is damaged: %s", (unsigned long long)b, (unsigned long long)at, id_error_text((uint32_t)e)); return HARC_AMD_EINVAL; }
        at += 4 + pb; tat += tb;
    }
    if (at != n_bytes) { harc_set_error("idunpack_host: block %llu ends at byte %llu, but there are %llu bytes", (unsigned long long)H.nb - 1, (unsigned long long)at, (unsigned long long)n_bytes); return HARC_AMD_EINVAL; }
    if (tat != H.text) { harc_set_error("idunpack_host: block %llu ends the text at byte %llu, the header announces %llu", (unsigned long long)H.nb - 1, (unsigned long long)tat, (unsigned long long)H.text); return HARC_AMD_EINVAL; }
    return HARC_AMD_OK;
}

// ------------------------------------------------------------------------------------------------ the files
namespace {
struct IpBuf { harc_amd_ctx *c; char *p = nullptr; size_t cap = 0; ~IpBuf() { if (p) harc_raw_free(c, p); } };
// at least `need` bytes, the first `keep` of them kept
int ip_reserve(IpBuf *b, size_t need, size_t keep)
{
    if (b->p && b->cap >= need) return HARC_AMD_OK;
    char *np = nullptr; const size_t cap = need + (keep ? need / 4 : 0);
    RC_TRY(harc_raw_alloc(b->c, (void **)&np, cap + 16));
    if (keep && hipMemcpyAsync(np, b->p, keep, hipMemcpyDeviceToDevice, b->c->stream) != hipSuccess) { harc_raw_free(b->c, np); harc_set_error("idpack_files: a device copy failed"); return HARC_AMD_ENODEVICE; }
    if (hipStreamSynchronize(b->c->stream) != hipSuccess) { harc_raw_free(b->c, np); harc_set_error("idpack_files: the device failed"); return HARC_AMD_ENODEVICE; }      // whatever still reads the old buffer has finished
    if (b->p) harc_raw_free(b->c, b->p);
    b->p = np; b->cap = cap;
    return HARC_AMD_OK;
}
bool ip_file_size(const char *path, uint64_t *n) { struct stat st; if (stat(path, &st) != 0 || !S_ISREG(st.st_mode)) return false; *n = (uint64_t)st.st_size; return true; }
struct IpOutGuard { std::string path; bool ok = false; ~IpOutGuard() { if (!ok) (void)remove(path.c_str()); } };
struct IpCtxGuard { harc_amd_ctx *c; ~IpCtxGuard() { harc_amd_destroy(c); } };
uint64_t ip_env_u64(const char *name, uint64_t dflt) { if (const char *e = getenv(name)) { const unsigned long long v = strtoull(e, nullptr, 10); if (v >= 1) return v; } return dflt; }
// the context's one pinned ring in two halves of eight slices: the feeder's and the drain's
int ip_ring(harc_amd_ctx *c, RingGeom *feed, RingGeom *drain)
{
    RingGeom base; harc_ring_geom_env(&base);
    for (RingGeom *g : { feed, drain }) { g->slice = base.slice; g->nslices = 8; g->nthr = base.nthr / 2 > 0 ? base.nthr / 2 : 1; }
    feed->ring_off = 0; drain->ring_off = 8 * base.slice;
    return harc_ring_reserve(c, 16 * base.slice, "id");
}
int ip_context(const harc_amd_params *params, harc_amd_ctx **c)
{
    harc_amd_params P = *params;
    if (harc_amd_default_params(100, &P) != HARC_AMD_OK) return HARC_AMD_EINVAL;
    P.device = params->device;
    return harc_amd_create(&P, c);
}
}

// The text goes through the ring in byte ranges of about `piece_blocks` blocks of ids of 80 bytes (4 KiB .. 256 MiB).  The line index of what has arrived says how
// many whole blocks it holds: they are packed, at most piece_blocks and at most IP_CALL_TEXT bytes of text a call (one block where a block alone is longer), and the
// rest is carried to the front of the next range, as fastq_out.hip carries a cut line.  The event scratch and the slabs are five bytes per byte of text: 1.25 GiB a
// call with ids of any length, and 5 GiB in the one case that cannot be cut, a single block of the 2^30 bytes a block may hold
extern "C" int harc_amd_idpack_files(const harc_amd_params *params, const char *id_path, const char *out_path)
{
    if (!params || !id_path || !out_path) { harc_set_error("idpack_files: bad arguments"); return HARC_AMD_EINVAL; }
    uint64_t isz = 0;
    if (!ip_file_size(id_path, &isz)) { harc_set_error("cannot open %s", id_path); return HARC_AMD_EIO; }
    IpOutGuard outguard{ out_path };
    if (isz) {                                                    // before a device is touched
        FILE *g = fopen(id_path, "rb"); char last = 0;
        if (!g || fseeko(g, (off_t)isz - 1, SEEK_SET) != 0 || fread(&last, 1, 1, g) != 1) { if (g) fclose(g); harc_set_error("cannot read %s", id_path); return HARC_AMD_EIO; }
        fclose(g);
        if (last != '\n') { harc_set_error("idpack_files: the last line of %s does not end in a newline", id_path); return HARC_AMD_EINVAL; }
    }
    const uint32_t rb = (uint32_t)ip_env_u64("HARC_AMD_IDPACK_BLOCK", ID_DEFAULT_RB);
    const uint64_t piece_blocks = ip_env_u64("HARC_AMD_IDPACK_PIECE", 8), call_text = ip_env_u64("HARC_AMD_IDPACK_CALL_TEXT", IP_CALL_TEXT);
    uint64_t piece = piece_blocks * rb * 80ull;
    if (piece < 4096) piece = 4096;
    if (piece > ((uint64_t)256 << 20)) piece = (uint64_t)256 << 20;
    harc_amd_ctx *c = nullptr;
    RC_TRY(ip_context(params, &c));
    IpCtxGuard guard{ c };
    RingGeom gf, gd;
    RC_TRY(ip_ring(c, &gf, &gd));
    IpBuf txt[2] = { { c }, { c } }, out{ c };
    const bool tlog = getenv("HARC_AMD_TRACE") != nullptr;
    double t_read = 0, t_write = 0;
    IpStats st;
    uint64_t at = ID_FILE_HEADER, n = 0, nb = 0; int npieces = 0;
    {
        FileDrain drain(c);
        RC_TRY(drain.start(out_path, (size_t)id_bound(isz, isz, rb), &gd, true));      // (no more lines than bytes)
        std::vector<std::pair<uint64_t, uint64_t>> pieces;
        for (uint64_t a = 0; a < isz; a += piece) pieces.emplace_back(a, isz - a < piece ? isz : a + piece);
        FileFeeder feed(c, id_path);
        if (!pieces.empty()) RC_TRY(feed.start(pieces, gf));
        uint64_t carry = 0; int cur = 0;
        for (size_t p = 0; p < pieces.size(); p++) {
            const uint64_t len = pieces[p].second - pieces[p].first, total = carry + len; const bool lastp = p + 1 == pieces.size();
            RC_TRY(ip_reserve(&txt[cur], (size_t)total, (size_t)carry));                     // the carried bytes sit at its front
            { const double t0 = mono_now(); RC_TRY(feed.upload_piece(p, txt[cur].p + carry, nullptr)); t_read += mono_now() - t0; }
            const char *d_ids = txt[cur].p;
            PoolScope piece_scope(c);
            const uint64_t *nls = nullptr; uint64_t lines = 0;
            RC_TRY(build_line_index(c, d_ids, total, &nls, &lines));
            if (!lastp) {                                                                    // an open last line counts as one: whole lines, then whole blocks
                char lastch = 0;
                HIP_TRY(hipMemcpyAsync(&lastch, d_ids + total - 1, 1, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                if (lastch != '\n') lines--;
                lines = lines / rb * rb;
            }
            uint64_t cut = 0;
            for (uint64_t l0 = 0; l0 < lines;) {
                // at most piece_blocks blocks a call and, by the line index, no more than IP_CALL_TEXT bytes of text unless one block alone is longer
                uint64_t m = lines - l0 < piece_blocks * rb ? lines - l0 : piece_blocks * rb, end = 0;
                for (;;) {
                    HIP_TRY(hipMemcpyAsync(&end, nls + (l0 + m - 1), 8, hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(hipStreamSynchronize(c->stream));
                    end += 1;
                    if (end - cut <= call_text || m <= rb) break;
                    const uint64_t half = (id_blocks(m, rb) / 2) * rb;
                    m = half < rb ? rb : half;
                }
                RC_TRY(ip_reserve(&out, (size_t)(id_bound(end - cut, m, rb) - ID_FILE_HEADER), 0));
                uint64_t nblk = 0;
                RC_TRY(harc_idpack_run(c, d_ids, nls + l0, cut, end, m, rb, (uint8_t *)out.p, out.cap, &nblk, nb, &st));
                { const double t0 = mono_now(); RC_TRY(drain.put(out.p, (size_t)nblk, at)); t_write += mono_now() - t0; }
                at += nblk; n += m; nb += id_blocks(m, rb); npieces++;
                l0 += m; cut = end;
            }
            const uint64_t rest = total - cut;
            if (rest && cut) {
                RC_TRY(ip_reserve(&txt[cur ^ 1], (size_t)rest, 0));
                HIP_TRY(hipMemcpyAsync(txt[cur ^ 1].p, d_ids + cut, (size_t)rest, hipMemcpyDeviceToDevice, c->stream));
                cur ^= 1;
            }
            carry = rest;
        }
        uint8_t h[ID_FILE_HEADER];
        id_file_header(h, rb, n, isz);
        RC_TRY(drain.put_host(h, ID_FILE_HEADER, 0));
        drain.set_final_size(at);
        { const double t0 = mono_now(); RC_TRY(drain.finish()); t_write += mono_now() - t0; }
    }
    if (tlog) fprintf(stderr, "[idpack] %llu bytes of text -> %llu bytes in %llu blocks (%llu stored), %d pieces: %.3f s in the kernels, %.3f s waiting for the readers, %.3f s waiting for the writers\n",
                      (unsigned long long)isz, (unsigned long long)at, (unsigned long long)nb, (unsigned long long)st.stored, npieces, st.seconds, t_read, t_write);
    outguard.ok = true;
    return HARC_AMD_OK;
}

extern "C" int harc_amd_idunpack_files(const harc_amd_params *params, const char *packed_path, const char *out_path)
{
    if (!params || !packed_path || !out_path) { harc_set_error("idunpack_files: bad arguments"); return HARC_AMD_EINVAL; }
    uint64_t fsz = 0;
    if (!ip_file_size(packed_path, &fsz)) { harc_set_error("cannot open %s", packed_path); return HARC_AMD_EIO; }
    IpOutGuard outguard{ out_path };
    if (fsz < ID_FILE_HEADER) { harc_set_error("idunpack_files: %s holds %llu bytes, fewer than the %u of the header", packed_path, (unsigned long long)fsz, ID_FILE_HEADER); return HARC_AMD_EINVAL; }
    const int fd = open(packed_path, O_RDONLY);
    if (fd < 0) { harc_set_error("cannot open %s", packed_path); return HARC_AMD_EIO; }
    struct FdGuard { int fd; ~FdGuard() { close(fd); } } fdguard{ fd };
    uint8_t h[ID_FILE_HEADER];
    if (pread(fd, h, ID_FILE_HEADER, 0) != (ssize_t)ID_FILE_HEADER) { harc_set_error("cannot read %s", packed_path); return HARC_AMD_EIO; }
    IdHeader H;
    RC_TRY(ip_parse_header("idunpack_files", h, fsz, &H));
    // the block offsets and the places in the text, from the prefixes: known, and inside the file, before a device is touched
    std::vector<uint64_t> off((size_t)H.nb + 1), toff((size_t)H.nb + 1);
    uint64_t at = ID_FILE_HEADER, tat = 0;
    for (uint64_t b = 0; b < H.nb; b++) {
        off[b] = at; toff[b] = tat;
        uint8_t q[4 + ID_HEAD0];
        if (fsz - at < sizeof q) { harc_set_error("idunpack_files: block %llu at byte %llu leaves the %llu bytes of %s", (unsigned long long)b, (unsigned long long)at, (unsigned long long)fsz, packed_path); return HARC_AMD_EINVAL; }
        if (pread(fd, q, sizeof q, (off_t)at) != (ssize_t)sizeof q) { harc_set_error("cannot read %s", packed_path); return HARC_AMD_EIO; }
        uint64_t pb = 0, tb = 0;
        RC_TRY(ip_check_prefix("idunpack_files", q, b, at, fsz, H.text - tat, &pb, &tb));
        at += 4 + pb; tat += tb;
    }
    off[H.nb] = at; toff[H.nb] = tat;
    if (at != fsz) { harc_set_error("idunpack_files: the blocks of %s end at byte %llu, the file holds %llu", packed_path, (unsigned long long)at, (unsigned long long)fsz); return HARC_AMD_EINVAL; }
    if (tat != H.text) { harc_set_error("idunpack_files: block %llu of %s ends the text at byte %llu, its header announces %llu", (unsigned long long)H.nb - 1, packed_path, (unsigned long long)tat, (unsigned long long)H.text); return HARC_AMD_EINVAL; }
    harc_amd_ctx *c = nullptr;
    RC_TRY(ip_context(params, &c));
    IpCtxGuard guard{ c };
    RingGeom gf, gd;
    RC_TRY(ip_ring(c, &gf, &gd));
    IpBuf pk{ c }, txt{ c }, doff{ c };
    const bool tlog = getenv("HARC_AMD_TRACE") != nullptr;
    double t_read = 0, t_write = 0, t_kernel = 0;
    const uint64_t piece_blocks = ip_env_u64("HARC_AMD_IDPACK_PIECE", 8);
    int npieces = 0;
    {
        FileDrain drain(c);
        RC_TRY(drain.start(out_path, (size_t)H.text, &gd, true));
        std::vector<std::pair<uint64_t, uint64_t>> pieces;
        for (uint64_t b = 0; b < H.nb; b += piece_blocks) pieces.emplace_back(off[b], off[H.nb - b < piece_blocks ? H.nb : b + piece_blocks]);
        FileFeeder feed(c, packed_path);
        if (!pieces.empty()) RC_TRY(feed.start(pieces, gf));
        std::vector<uint64_t> rel;
        for (size_t p = 0; p < pieces.size(); p++) {
            const uint64_t b0 = p * piece_blocks, b1 = H.nb - b0 < piece_blocks ? H.nb : b0 + piece_blocks, bytes = pieces[p].second - pieces[p].first, k = b1 - b0 + 1;
            const uint64_t line0 = b0 * H.rb, m = (b1 == H.nb ? H.n : b1 * H.rb) - line0, tbytes = toff[b1] - toff[b0];
            RC_TRY(ip_reserve(&pk, (size_t)bytes, 0)); RC_TRY(ip_reserve(&txt, (size_t)tbytes + 1, 0)); RC_TRY(ip_reserve(&doff, 16 * (size_t)k, 0));
            { const double t0 = mono_now(); RC_TRY(feed.upload_piece(p, pk.p, nullptr)); t_read += mono_now() - t0; }
            rel.resize((size_t)(2 * k));
            for (uint64_t b = b0; b <= b1; b++) { rel[(size_t)(b - b0)] = off[b] - off[b0]; rel[(size_t)(k + b - b0)] = toff[b] - toff[b0]; }
            HIP_TRY(hipMemcpyAsync(doff.p, rel.data(), 8 * rel.size(), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            { const double t0 = mono_now(); RC_TRY(harc_idunpack_run(c, (const uint8_t *)pk.p, (const uint64_t *)doff.p, (const uint64_t *)doff.p + k, rel.data(), (uint32_t)(b1 - b0), m, H.rb, txt.p, b0, off[b0])); t_kernel += mono_now() - t0; }
            { const double t0 = mono_now(); RC_TRY(drain.put(txt.p, (size_t)tbytes, toff[b0])); t_write += mono_now() - t0; }
            npieces++;
        }
        drain.set_final_size(H.text);
        { const double t0 = mono_now(); RC_TRY(drain.finish()); t_write += mono_now() - t0; }
    }
    if (tlog) fprintf(stderr, "[idpack] unpacked %llu bytes of text from %llu bytes in %llu blocks, %d pieces: %.3f s in the kernels, %.3f s waiting for the readers, %.3f s waiting for the writers\n",
                      (unsigned long long)H.text, (unsigned long long)fsz, (unsigned long long)H.nb, npieces, t_kernel, t_read, t_write);
    outguard.ok = true;
    return HARC_AMD_OK;
}
