// bgzf_out.hip -- text in device memory -> BGZF (SAM/BAM specification 4.1) in device memory: the way ./harc -d -q -z writes X.d.fastq.gz, a file that ./harc -c,
// bgzip -d, gzip -d and samtools read.  The text is cut every DM_TEXT = 65 280 bytes; a workgroup deflates one member by the rules of deflate_member.h (matches
// only against the line four lines up at the same column: no search, every byte decides for itself), one dynamic Huffman block or a stored one.
//
// Sizes are needed before bytes can be placed.  Of the two ways -- plan (tokens, histograms, codes, sizes), scan, emit; or emit into 64-KiB slots, scan, compact --
// this is the second: the plan is most of the work (every pass over the text and the three Huffman codes) and would be done twice, while compaction reads and
// writes the COMPRESSED bytes once more, about a quarter of the text for FASTQ.  k_bgzf_deflate writes member i to slot i of a scratch buffer and its size to a
// table; the sizes are scanned (prims.hip); k_bgzf_compact moves every member to its place, whatever the alignment of the output, and appends the marker.
//
// k_bgzf_deflate, 1024 lanes, lane t owns the 64 bytes [64 t, 64 t + 64) of the member.  The text is staged in LDS once (it is walked five times and every walk
// also reads text[j - D]); rows of 16 dwords are padded to 17, so that the lanes of a wave, 64 bytes apart, read 64 different banks.  With the bit stream
// (64 KiB) that is 141 KiB of the CU's 160: one workgroup per CU, 4 waves per SIMD.  Per lane the member is 64-bit masks: newlines, equal bytes, run breaks.
//   1 newlines and the chunk's CRC-32; newline counts scanned over the workgroup                     4 histograms, LDS atomics
//   2 the five line starts in front of the chunk (binary search in the scanned counts), equal bytes  5 three Huffman codes: sorted by rank, a lane per code
//   3 run breaks; the break before and behind the chunk through one ballot per wave                  6 token bits scanned over the workgroup, bits OR-ed into LDS
//   7 the chunk CRCs folded as a tree of products with x^(512 * 2^level); header, stream or stored text and trailer leave in 16-byte stores
#include "devutil.h"
#include "deflate_member.h"
#include "fileio.h"                                               // KernelTimer

#define BZ_T 1024
#define BZ_ROW 17                        // dwords per 64-byte row of the text in LDS
#define BZ_SLOT 65536u                   // scratch bytes per member (DM_MEMBER_MAX = 65 311 rounded up)

struct BzShared {
    uint32_t text[BZ_T * BZ_ROW];
    uint32_t obuf[16384];                // the DEFLATE stream; a dynamic block is kept only when it is shorter than the text + 5
    DmCodes w;
    uint64_t nlmask[BZ_T];
    uint64_t wmask[BZ_T / 64];
    uint32_t cum[BZ_T + 1];              // newlines in front of every chunk; later the CRC tree
    uint32_t crctab[256];
    uint32_t scan[BZ_T / 64 + 1];
    uint32_t crc_last, crc;
    uint16_t lastb[BZ_T], firstb[BZ_T];  // last / first run break of every chunk (0xFFFF: none)
    uint8_t eqtop[BZ_T], chg0[BZ_T + 1];
};

__device__ __forceinline__ uint32_t bz_tb(const uint8_t *t8, uint32_t j) { return t8[(j >> 6) * (BZ_ROW * 4) + (j & 63u)]; }

struct BzEmit { uint32_t *obuf; uint32_t w; uint64_t acc; int cnt; };
__device__ __forceinline__ void bz_put(BzEmit &e, uint32_t v, int n)      // n <= 28
{
    e.acc |= (uint64_t)v << e.cnt; e.cnt += n;
    if (e.cnt >= 32) { atomicOr(&e.obuf[e.w++], (uint32_t)e.acc); e.acc >>= 32; e.cnt -= 32; }
}

// One walk over the lane's chunk.  MODE 0: histograms; 1: -> bits of its tokens; 2: the bits into the stream.
template <int MODE>
__device__ __forceinline__ uint32_t bz_walk(BzShared &S, const uint8_t *t8, uint32_t j0, uint32_t cnt, uint64_t eqm, uint64_t brk, uint32_t prevLast, uint32_t nextFirst,
                                            uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t a4, BzEmit *em)
{
    uint32_t bits = 0, D = dm_D(a0, a4);
    const uint8_t *row = t8 + (j0 >> 6) * (BZ_ROW * 4);
    for (uint32_t b = 0; b < cnt; b++) {
        const uint32_t j = j0 + b, c = row[b];
        uint32_t len = 0; bool lit = true;
        if ((eqm >> b) & 1ull) {
            const uint64_t low = brk & (b == 63 ? ~0ull : ((2ull << b) - 1ull)), high = b == 63 ? 0ull : brk & (~0ull << (b + 1));
            const uint32_t s = low ? j0 + 63u - (uint32_t)__clzll((long long)low) : prevLast, e = high ? j0 + (uint32_t)__ffsll((long long)high) - 1u : nextFirst;
            const uint32_t R = e - s;
            if (R >= DM_MINRUN) { lit = false; len = dm_piece(R, j - s); }
        }
        if (lit) {
            if (MODE == 0) atomicAdd(&S.w.lfreq[c], 1u);
            else if (MODE == 1) bits += S.w.llen[c];
            else bz_put(*em, S.w.lcode[c], S.w.llen[c]);
        } else if (len) {
            if (MODE == 0) { atomicAdd(&S.w.lfreq[257 + dm_lsym(len)], 1u); atomicAdd(&S.w.dfreq[dm_dsym(D)], 1u); }
            else {
                int n1, n2; const uint32_t v1 = dm_len_bits(S.w, len, &n1), v2 = dm_dist_bits(S.w, D, &n2);
                if (MODE == 1) bits += (uint32_t)(n1 + n2);
                else { bz_put(*em, v1, n1); bz_put(*em, v2, n2); }
            }
        }
        if (c == '\n') { a4 = a3; a3 = a2; a2 = a1; a1 = a0; a0 = j + 1; D = dm_D(a0, a4); }
    }
    return bits;
}

// the position of newline number m of the member (m < the member's newlines), from the scanned counts and the masks of the chunks
__device__ __forceinline__ uint32_t bz_nlpos(const BzShared &S, uint32_t m, uint32_t hi)
{
    uint32_t lo = 0;
    while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (S.cum[mid] <= m) lo = mid; else hi = mid - 1; }
    uint64_t mk = S.nlmask[lo];
    for (uint32_t r = m - S.cum[lo]; r; r--) mk &= mk - 1;
    return lo * 64u + (uint32_t)__ffsll((long long)mk) - 1u;
}
// start of the line i lines in front of line k: 0 for the member's first line, DM_NONE in front of it
__device__ __forceinline__ uint32_t bz_line_start(const BzShared &S, uint32_t k, uint32_t i, uint32_t t)
{
    if (k < i) return DM_NONE;
    return k == i ? 0u : bz_nlpos(S, k - i - 1, t) + 1u;
}

// member mi = text[mi * DM_TEXT ..) -> slots + mi * BZ_SLOT, its size -> msize[mi].  stat[0]: stored members; stat[1]: members whose bit count disagrees with
// the cost computed from the histograms (never: an internal error)
__global__ __launch_bounds__(BZ_T) void k_bgzf_deflate(const char *text, uint64_t n_bytes, uint32_t nm, uint8_t *slots, uint32_t *msize, unsigned int *stat)
{
    __shared__ __attribute__((aligned(16))) BzShared S;
    const uint64_t mi = harc_bid();
    if (mi >= nm) return;
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const uint64_t base = mi * (uint64_t)DM_TEXT;
    const uint32_t n = n_bytes - base < DM_TEXT ? (uint32_t)(n_bytes - base) : DM_TEXT;
    const uint8_t *t8 = (const uint8_t *)S.text;
    {   // the text into LDS by aligned dwords, whatever the alignment of the input; nothing outside the dwords that hold its bytes is read
        const uintptr_t u = (uintptr_t)(text + base);
        const uint32_t sh = (uint32_t)(u & 3), ndw = (n + 3) >> 2;
        const uint32_t *wsrc = (const uint32_t *)(u - sh);
        for (uint32_t g = t; g < BZ_T * 16; g += BZ_T) {
            uint32_t v = 0;
            if (g < ndw) {
                const uint32_t lo = wsrc[g];
                uint32_t hi = 0;
                if (sh && 4 * g + 4 - sh < n) hi = wsrc[g + 1];
                v = __builtin_amdgcn_alignbyte(hi, lo, sh);
            }
            S.text[(g >> 4) * BZ_ROW + (g & 15u)] = v;
        }
        for (uint32_t g = t; g < 16384; g += BZ_T) S.obuf[g] = 0;
        if (t < DM_NLL) { S.w.lfreq[t] = t == 256 ? 1u : 0u; S.w.llen[t] = 0; }
        if (t < DM_ND) S.w.dfreq[t] = 0;
        if (t < DM_ND + 2) S.w.dlen[t] = 0;
        if (t < 256) S.crctab[t] = im_crc_entry(t);
        if (t == 0) S.chg0[0] = 0;
    }
    __syncthreads();
    const uint32_t j0 = t * 64u, cnt = j0 < n ? (n - j0 < 64u ? n - j0 : 64u) : 0u;
    const uint8_t *row = t8 + t * (BZ_ROW * 4);
    // ---- 1: newlines, CRC of the chunk
    uint64_t nl = 0; uint32_t crc = 0xFFFFFFFFu;
    for (uint32_t b = 0; b < cnt; b++) {
        const uint32_t c = row[b];
        nl |= (uint64_t)(c == '\n') << b;
        crc = S.crctab[(crc ^ c) & 0xFFu] ^ (crc >> 8);
    }
    crc ^= 0xFFFFFFFFu;                                            // (0 for a chunk without bytes)
    S.nlmask[t] = nl;
    uint32_t nltot;
    const uint32_t k = block_excl_scan_u32<BZ_T>((uint32_t)__popcll(nl), S.scan, &nltot);      // newlines in front of the chunk = the line its first byte is in
    S.cum[t] = k;
    if (t == 0) S.cum[BZ_T] = nltot;
    __syncthreads();
    // ---- 2: the line starts in front of the chunk, then the equal bytes and where the distance changes
    const uint32_t s0 = bz_line_start(S, k, 0, t), s1 = bz_line_start(S, k, 1, t), s2 = bz_line_start(S, k, 2, t), s3 = bz_line_start(S, k, 3, t),
                   s4 = bz_line_start(S, k, 4, t);
    uint64_t eqm = 0, chg = 0; uint32_t carry = 0;
    {
        uint32_t a0 = s0, a1 = s1, a2 = s2, a3 = s3, a4 = s4, D = dm_D(a0, a4);
        for (uint32_t b = 0; b < cnt; b++) {
            const uint32_t j = j0 + b, c = row[b];
            if (D && c == bz_tb(t8, j - D)) eqm |= 1ull << b;
            if (c == '\n') {
                const uint32_t Dn = dm_D(j + 1, a3);
                if (Dn != D) { if (b < 63) chg |= 2ull << b; else carry = 1; }
                a4 = a3; a3 = a2; a2 = a1; a1 = a0; a0 = j + 1; D = Dn;
            }
        }
    }
    S.eqtop[t] = (uint8_t)(eqm >> 63);
    S.chg0[t + 1] = (uint8_t)carry;
    __syncthreads();
    // ---- 3: a byte breaks a run unless it and the byte in front of it are equal bytes of one distance
    const uint64_t valid = cnt == 64 ? ~0ull : ((1ull << cnt) - 1ull);
    const uint64_t brk = (~(eqm & ((eqm << 1) | (uint64_t)(t ? S.eqtop[t - 1] : 0))) | chg | (uint64_t)S.chg0[t]) & valid;
    S.lastb[t] = brk ? (uint16_t)(j0 + 63u - (uint32_t)__clzll((long long)brk)) : (uint16_t)0xFFFF;
    S.firstb[t] = brk ? (uint16_t)(j0 + (uint32_t)__ffsll((long long)brk) - 1u) : (uint16_t)0xFFFF;
    const uint64_t wm = __ballot(brk != 0);
    if (lane == 0) S.wmask[wv] = wm;
    __syncthreads();
    uint32_t prevLast = 0, nextFirst = n;
    {
        uint64_t m = wm & ((1ull << lane) - 1ull); int w = (int)wv;
        while (!m && w > 0) m = S.wmask[--w];
        if (m) prevLast = S.lastb[w * 64 + 63 - __clzll((long long)m)];
        m = lane == 63 ? 0ull : wm & (~0ull << (lane + 1)); w = (int)wv;
        while (!m && w < BZ_T / 64 - 1) m = S.wmask[++w];
        if (m) nextFirst = S.firstb[w * 64 + __ffsll((long long)m) - 1];
    }
    // ---- 4: histograms
    (void)bz_walk<0>(S, t8, j0, cnt, eqm, brk, prevLast, nextFirst, s0, s1, s2, s3, s4, nullptr);
    __syncthreads();
    // ---- 5: the codes.  Symbols sorted by rank, a lane each; then one lane per code for the lengths; then one lane for the header
    if (t < DM_NLL) { const uint32_t f = S.w.lfreq[t]; if (f) { const uint32_t r = dm_rank(S.w.lfreq, DM_NLL, (int)t); S.w.lsrt[r] = (uint16_t)t; S.w.lA[r] = f; } }
    else if (t >= 512 && t < 512 + DM_ND) { const uint32_t s = t - 512, f = S.w.dfreq[s]; if (f) { const uint32_t r = dm_rank(S.w.dfreq, DM_ND, (int)s); S.w.dsrt[r] = (uint16_t)s; S.w.dA[r] = f; } }
    __syncthreads();
    if (t == 0) { int used = 0; for (int s = 0; s < DM_NLL; s++) used += S.w.lfreq[s] != 0; dm_lengths_sorted(S.w.lA, S.w.lsrt, used, 15, S.w.llen, S.w.blc[0]); }
    else if (t == 64) { int used = 0; for (int s = 0; s < DM_ND; s++) used += S.w.dfreq[s] != 0; dm_lengths_sorted(S.w.dA, S.w.dsrt, used, 15, S.w.dlen, S.w.blc[1]); }
    __syncthreads();
    if (t == 0) {
        dm_finish_codes(S.w, n);
        if (!S.w.stored) {
            DmBits hb; hb.out = (uint8_t *)S.obuf; hb.pos = 0; hb.acc = 0; hb.cnt = 0;
            dm_put_header(hb, S.w);
            dm_flush(hb);                                          // the last byte is shared with the first token: its lanes OR their bits in
        }
    }
    __syncthreads();
    const uint32_t stored = S.w.stored, tlast = (n - 1) >> 6;
    // ---- 6: the bit stream
    if (!stored) {
        uint32_t bits = bz_walk<1>(S, t8, j0, cnt, eqm, brk, prevLast, nextFirst, s0, s1, s2, s3, s4, nullptr);
        if (t == tlast) bits += S.w.llen[256];
        uint32_t tot;
        const uint32_t at = S.w.hdr_bits + block_excl_scan_u32<BZ_T>(bits, S.scan, &tot);
        if (t == 0 && S.w.hdr_bits + tot != S.w.total_bits) atomicAdd(&stat[1], 1u);
        BzEmit em; em.obuf = S.obuf; em.w = at >> 5; em.acc = 0; em.cnt = (int)(at & 31u);
        (void)bz_walk<2>(S, t8, j0, cnt, eqm, brk, prevLast, nextFirst, s0, s1, s2, s3, s4, &em);
        if (t == tlast) bz_put(em, S.w.lcode[256], S.w.llen[256]);
        if (em.acc) atomicOr(&S.obuf[em.w], (uint32_t)em.acc);
    }
    // ---- 7: CRC-32 of the member: the full chunks right-aligned in a tree (a chunk that is not there counts as no bytes: CRC 0), then the last chunk
    __syncthreads();
    if (t < tlast) S.cum[t + BZ_T - tlast] = crc; else S.cum[t - tlast] = 0;
    if (t == tlast) S.crc_last = crc;
    uint32_t Xp = dm_xpow8(DM_CRC_CHUNK);
    for (uint32_t half = BZ_T / 2; half >= 1; half >>= 1) {
        __syncthreads();
        uint32_t v = 0;
        if (t < half) v = dm_gfmul(S.cum[2 * t], Xp) ^ S.cum[2 * t + 1];
        __syncthreads();
        if (t < half) S.cum[t] = v;
        Xp = dm_gfmul(Xp, Xp);
    }
    __syncthreads();
    if (t == 0) S.crc = dm_gfmul(S.cum[0], dm_xpow8(n - tlast * 64u)) ^ S.crc_last;
    __syncthreads();
    // ---- the member: header, CDATA (the stream, or five bytes and the text), CRC-32, ISIZE
    const uint32_t clen = stored ? n + 5 : (S.w.total_bits + 7) >> 3, size = 18 + clen + 8, crcm = S.crc;
    const uint8_t *o8 = (const uint8_t *)S.obuf;
    uint8_t *slot = slots + mi * (uint64_t)BZ_SLOT;
    for (uint32_t q = t; q * 16 < size; q += BZ_T) {
        uint32_t v[4];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            uint32_t x = 0;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                uint32_t kk = q * 16 + d * 4 + e, byte;
                if (kk < 18) byte = dm_header_byte(kk, size - 1);
                else if ((kk -= 18) < clen) byte = stored ? (kk < 5 ? dm_stored_byte(kk, n) : bz_tb(t8, kk - 5)) : o8[kk];
                else if ((kk -= clen) < 4) byte = (crcm >> (8 * kk)) & 0xFFu;
                else if (kk < 8) byte = (n >> (8 * (kk - 4))) & 0xFFu;
                else byte = 0;
                x |= byte << (8 * e);
            }
            v[d] = x;
        }
        *(uint4 *)(slot + 16 * q) = make_uint4(v[0], v[1], v[2], v[3]);
    }
    if (t == 0) { msize[mi] = size; if (stored) atomicAdd(&stat[0], 1u); }
}

// member mi from its slot to out + moff[mi]; workgroup nm writes the end-of-file marker behind the last member.  Only bytes of the members are written: the
// dwords of the destination that lie inside a member whole, the bytes in front of and behind them one by one
__global__ __launch_bounds__(256) void k_bgzf_compact(const uint8_t *slots, const uint32_t *msize, const uint64_t *moff, uint32_t nm, int eof, uint8_t *out)
{
    const uint64_t mi = harc_bid();
    if (mi > nm || (mi == nm && !eof)) return;
    const uint32_t t = threadIdx.x;
    uint8_t *dst = out + moff[mi];
    if (mi == nm) { if (t < 28) dst[t] = dm_eof_byte(t); return; }
    const uint32_t len = msize[mi];
    const uint8_t *src = slots + mi * (uint64_t)BZ_SLOT;
    uint32_t head = (uint32_t)((0 - (uintptr_t)dst) & 3);
    if (head > len) head = len;
    if (t < head) dst[t] = src[t];
    const uint32_t nd = (len - head) >> 2, sh = head & 3u;
    for (uint32_t i = t; i < nd; i += 256) {
        const uint32_t kk = head + 4 * i;                           // the slot is BZ_SLOT bytes: the dword behind a member's last byte is inside it
        const uint32_t *sw = (const uint32_t *)(src + (kk & ~3u));
        *(uint32_t *)(dst + kk) = sh ? __builtin_amdgcn_alignbyte(sw[1], sw[0], sh) : sw[0];
    }
    const uint32_t done = head + 4 * nd;
    if (t < len - done) dst[done + t] = src[done + t];
}

int harc_bgzf_deflate(harc_amd_ctx *c, const char *d_text, uint64_t n_bytes, int32_t flags, uint8_t *d_out, uint64_t out_capacity, uint64_t *n_out, BgzfOutStats *st)
{
    const uint64_t nm64 = (n_bytes + DM_TEXT - 1) / DM_TEXT;
    if (nm64 > 0xFFFFFFF0ull) { harc_set_error("bgzf_deflate: too much text for one call"); return HARC_AMD_EINVAL; }
    const uint32_t nm = (uint32_t)nm64; const bool eof = (flags & 1) != 0;
    PoolScope scope(c);
    uint8_t *slots = nullptr; uint32_t *msize = nullptr; uint64_t *moff = nullptr; unsigned int *d_stat = nullptr;
    RC_TRY(dalloc(c, &slots, (size_t)nm * BZ_SLOT)); RC_TRY(dalloc(c, &msize, (size_t)nm + 1)); RC_TRY(dalloc(c, &moff, (size_t)nm + 1)); RC_TRY(dalloc(c, &d_stat, 4));
    HIP_TRY(hipMemsetAsync(msize + nm, 0, 4, c->stream));
    HIP_TRY(hipMemsetAsync(d_stat, 0, 16, c->stream));
    KernelTimer timer(st ? &st->seconds : nullptr);
    RC_TRY(timer.begin(c->stream));
    if (nm) {
        hipLaunchKernelGGL(k_bgzf_deflate, harc_fold256(nm), dim3(BZ_T), 0, c->stream, d_text, n_bytes, nm, slots, msize, d_stat);
        HIP_TRY(hipGetLastError());
    }
    RC_TRY(prim_excl_scan_u32_to_u64(c, msize, moff, (size_t)nm + 1));
    uint64_t members_bytes = 0; unsigned int stat[2] = { 0, 0 };
    HIP_TRY(hipMemcpyAsync(&members_bytes, moff + nm, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(stat, d_stat, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (stat[1]) { harc_set_error("bgzf_deflate: %u members whose bit count differs from the cost of their codes", stat[1]); return HARC_AMD_EINTERNAL; }
    const uint64_t total = members_bytes + (eof ? 28 : 0);
    *n_out = total;
    if (st) { st->text += n_bytes; st->bytes += total; st->members += nm; st->stored += stat[0]; }
    if (!d_out) return HARC_AMD_OK;
    if (out_capacity < total) {
        harc_set_error("bgzf_deflate_device: the members take %llu bytes, the buffer holds %llu", (unsigned long long)total, (unsigned long long)out_capacity);
        return HARC_AMD_EINVAL;
    }
    if (nm || eof) {
        hipLaunchKernelGGL(k_bgzf_compact, harc_fold256((uint64_t)nm + 1), dim3(256), 0, c->stream, (const uint8_t *)slots, (const uint32_t *)msize, (const uint64_t *)moff,
                           nm, eof ? 1 : 0, d_out);
        HIP_TRY(hipGetLastError());
    }
    RC_TRY(timer.end(c->stream));
    return HARC_AMD_OK;
}

extern "C" uint64_t harc_amd_bgzf_bound(uint64_t n_text) { return dm_bound(n_text); }

extern "C" int harc_amd_bgzf_deflate_device(harc_amd_ctx *c, const char *d_text, uint64_t n_bytes, int32_t flags, uint8_t *d_out, uint64_t out_capacity, uint64_t *n_out)
{
    if (!c || (n_bytes && !d_text) || !n_out) { harc_set_error("bgzf_deflate_device: bad arguments"); return HARC_AMD_EINVAL; }
    HIP_TRY(hipSetDevice(c->P.device));
    if (!getenv("HARC_AMD_TRACE")) return harc_bgzf_deflate(c, d_text, n_bytes, flags, d_out, out_capacity, n_out, nullptr);
    BgzfOutStats st;
    const int rc = harc_bgzf_deflate(c, d_text, n_bytes, flags, d_out, out_capacity, n_out, &st);
    if (rc == HARC_AMD_OK) fprintf(stderr, "[bgzf_out] device call: %llu bytes of text -> %llu bytes in %llu members (%llu stored), deflate kernels %.3f ms (%.1f GB/s of text)\n",
                                   (unsigned long long)st.text, (unsigned long long)st.bytes, (unsigned long long)st.members, (unsigned long long)st.stored, 1e3 * st.seconds,
                                   st.seconds > 0 ? 1e-9 * (double)st.text / st.seconds : 0.0);
    return rc;
}

// the encoder of deflate_member.h run in a row on the host: what the kernels must write, byte for byte (tests)
extern "C" int harc_amd_bgzf_deflate_host(const char *text, uint64_t n_bytes, int32_t flags, uint8_t *out, uint64_t out_capacity, uint64_t *n_out)
{
    if ((n_bytes && !text) || !out || !n_out) { harc_set_error("bgzf_deflate_host: bad arguments"); return HARC_AMD_EINVAL; }
    if (out_capacity < dm_bound(n_bytes)) { harc_set_error("bgzf_deflate_host: the buffer holds %llu bytes, %llu may be needed", (unsigned long long)out_capacity, (unsigned long long)dm_bound(n_bytes)); return HARC_AMD_EINVAL; }
    std::vector<uint32_t> crctab(256);
    for (uint32_t i = 0; i < 256; i++) crctab[i] = im_crc_entry(i);
    std::vector<DmHost> H(1);
    uint64_t at = 0;
    for (uint64_t a = 0; a < n_bytes; a += DM_TEXT)
        at += dm_member((const uint8_t *)text + a, n_bytes - a < DM_TEXT ? (uint32_t)(n_bytes - a) : DM_TEXT, out + at, H[0], crctab.data());
    if (flags & 1) for (uint32_t k = 0; k < 28; k++) out[at++] = dm_eof_byte(k);
    *n_out = at;
    return HARC_AMD_OK;
}
