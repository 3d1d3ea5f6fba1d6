// ingest.hip -- FASTQ ingest on the GPU: the work of src/preprocess.cpp:81-121 (take line 2 of every
// 4-line record, check the fixed read length, split reads with and without N, remember the original index of every N read) and of
// readDnaFile / stringtobitset (reorder.cpp:240-263,203-209) without the single-threaded getline loop and without the
// input_clean.dna round trip: the whole file is staged in HBM, a prefix sum over the newline flags gives the line index, one thread
// per record classifies, two compactions pack the reads straight into the 2-bit / 3-bit stores of the context.
#include "devutil.h"
#include "inflate_member.h"
#include "fileio.h"
#include "check_block.h"
#include "third.h"

// line index in two levels: newlines per 4096-byte tile -> scan of the tile counts -> positions written tile by tile
#define NL_TILE 4096
__device__ __forceinline__ uint32_t nl_count16(const char *txt, uint64_t n, uint64_t at, uint32_t *mask)
{
    uint32_t m = 0;
    for (int k = 0; k < 16; k++) if (at + k < n && txt[at + k] == '\n') m |= 1u << k;
    *mask = m;
    return (uint32_t)__popc(m);
}
__global__ __launch_bounds__(256) void k_nl_count(const char *txt, uint64_t n, uint32_t *tilecnt)
{
    __shared__ uint32_t sm[8];
    const uint64_t at = (uint64_t)blockIdx.x * NL_TILE + (uint64_t)threadIdx.x * 16;
    uint32_t m; uint32_t cnt = nl_count16(txt, n, at, &m);
    uint32_t tot; (void)block_excl_scan_u32<256>(cnt, sm, &tot);
    if (threadIdx.x == 0) tilecnt[blockIdx.x] = tot;
}
__global__ __launch_bounds__(256) void k_nl_write(const char *txt, uint64_t n, const uint64_t *tilebase, uint64_t *nl)
{
    __shared__ uint32_t sm[8];
    const uint64_t at = (uint64_t)blockIdx.x * NL_TILE + (uint64_t)threadIdx.x * 16;
    uint32_t m; uint32_t cnt = nl_count16(txt, n, at, &m);
    uint32_t tot; const uint32_t off = block_excl_scan_u32<256>(cnt, sm, &tot);
    uint64_t o = tilebase[blockIdx.x] + off;
    while (m) { const int k = __ffs((int)m) - 1; m &= m - 1; nl[o++] = at + k; }
}
// record r = lines 4r .. 4r+3 ; sequence = line 4r+1 = bytes (nl[4r], nl[4r+1]).  flags: bit0 = has N, err counts bad lengths
__global__ void k_classify(const char *txt, const uint64_t *nl, uint32_t nrec, int L, uint32_t *isN, uint32_t *isClean, unsigned int *err)
{
    const uint32_t r = harc_gid32();
    if (r >= nrec) return;
    const uint64_t s = nl[4ull * r] + 1, e = nl[4ull * r + 1];
    uint64_t len = e - s;
    if (len && txt[e - 1] == '\r') len--;                         // tolerate CRLF
    if (len != (uint64_t)L) { atomicAdd(err, 1u); isN[r] = 0; isClean[r] = 0; return; }    // preprocess.cpp:92-97
    bool hasN = false;
    for (int j = 0; j < L; j++) hasN |= txt[s + j] == 'N';        // preprocess.cpp:98
    isN[r] = hasN ? 1u : 0u; isClean[r] = hasN ? 0u : 1u;
}
// clean reads -> 2-bit words (one thread per (record, word)); N reads -> 3-bit words; original index of N reads (read_order_N.bin)
__global__ void k_ingest_pack2(const char *txt, const uint64_t *nl, const uint32_t *isClean, const uint32_t *rankC, uint32_t nrec, int L, int W, uint64_t *out)
{
    const uint64_t gid = harc_gid();
    if (gid >= (uint64_t)nrec * W) return;
    const uint32_t r = (uint32_t)(gid / W); const int w = (int)(gid % W);
    if (!isClean[r]) return;
    const char *s = txt + nl[4ull * r] + 1;
    uint64_t v = 0;
    for (int k = 0; k < 32; k++) {
        const int b = 32 * w + k;
        if (b < L) { const char ch = s[b]; v |= (uint64_t)(ch == 'A' ? 0 : ch == 'G' ? 1 : ch == 'C' ? 2 : 3) << (2 * k); }
    }
    out[(size_t)rankC[r] * W + w] = v;
}
__global__ void k_ingest_pack3(const char *txt, const uint64_t *nl, const uint32_t *isN, const uint32_t *rankN, uint32_t nrec, int L, int W3, uint64_t *out, uint32_t *orderN)
{
    const uint64_t gid = harc_gid();
    if (gid >= (uint64_t)nrec * W3) return;
    const uint32_t r = (uint32_t)(gid / W3); const int w = (int)(gid % W3);
    if (!isN[r]) return;
    const char *s = txt + nl[4ull * r] + 1;
    uint64_t v = 0;
    const int b0 = (64 * w) / 3, b1 = (64 * w + 63) / 3;
    for (int b = b0; b <= b1 && b < L; b++) {
        const char ch = s[b];
        const uint64_t c3 = ch == 'A' ? 0 : ch == 'N' ? 1 : ch == 'G' ? 2 : ch == 'C' ? 4 : 6;
        const int sh = 3 * b - 64 * w;
        v |= sh >= 0 ? (c3 << sh) : (c3 >> (-sh));
    }
    out[(size_t)rankN[r] * W3 + w] = v;
    if (w == 0) orderN[rankN[r]] = r;                             // preprocess.cpp:102
}

// ---- the rule of the third lines (third.h), found while the piece is here anyway (-q only).  TH_G lanes per record; a lane takes 8 bytes of the id line and of
// the third line per step, through aligned 8-byte loads funnelled into place: the two lines sit at unrelated alignments of the same text.  A third line of
// length 1 is decided from the line index and its single byte, so that a file with bare third lines reads no id text at all.  Every lane holds the flags its own
// bytes leave standing, the wave ANDs them with two ballots and issues at most one atomicAnd -- none once the word holds no bit that the wave would clear.
#define TH_G 8
// the k (1 .. 8) bytes at p, the others zero; only aligned words that hold one of them are read
__device__ __forceinline__ uint64_t th_fetch8(const uint8_t *p, uint32_t k)
{
    const uintptr_t u = (uintptr_t)p;
    const uint32_t sh = (uint32_t)(u & 7);
    const uint64_t *w = (const uint64_t *)(u - sh);
    uint64_t v = w[0] >> (8 * sh);
    if (sh + k > 8) v |= w[1] << (64 - 8 * sh);                   // (sh > 0 here)
    if (k < 8) v &= ((uint64_t)1 << (8 * k)) - 1;
    return v;
}
// record r of the piece: id line (nl[4r-1], nl[4r]), third line (nl[4r+1], nl[4r+2]).  *flags &= the flags of every record
__global__ __launch_bounds__(256) void k_third_rule(const uint8_t *txt, const uint64_t *nl, uint64_t nrec, unsigned int *flags)
{
    const uint64_t r = harc_gid() / TH_G;
    const uint32_t g = threadIdx.x & (TH_G - 1);
    uint32_t f = TH_F_ALL;
    if (r < nrec) {
        const uint64_t a0 = nl[4 * (int64_t)r - 1] + 1, la = nl[4 * r] - a0, t0 = nl[4 * r + 1] + 1, lt = nl[4 * r + 2] - t0;
        if (lt == 1) { if (g == 0) f = th_flags_short(txt[t0], la); else f = TH_F_BARE | (la == 1 ? TH_F_SAME : 0u); }
        else if (lt == 0 || lt != la) f = 0;
        else {
            f = TH_F_SAME;
            const uint8_t *pa = txt + a0, *pt = txt + t0;
            const uint32_t len = (uint32_t)la;
            for (uint32_t off = 8 * g; off < len; off += 8 * TH_G) {
                const uint32_t k = len - off < 8 ? len - off : 8;
                const uint64_t vt = th_fetch8(pt + off, k);
                uint64_t x = th_fetch8(pa + off, k) ^ vt;
                if (off == 0) { x &= ~(uint64_t)0xFF; if ((vt & 0xFF) != (uint64_t)'+') f = 0; }     // a[0] is not looked at, t[0] is the '+'
                if (x) f = 0;
            }
        }
    }
    const uint32_t fw = (__ballot(!(f & TH_F_BARE)) ? 0u : TH_F_BARE) | (__ballot(!(f & TH_F_SAME)) ? 0u : TH_F_SAME);
    if ((threadIdx.x & 63u) == 0 && (*(volatile unsigned int *)flags & ~fw & TH_F_ALL) != 0) atomicAnd(flags, fw);
}

#define G256(n) harc_grid256((uint64_t)(n)), dim3(256), 0, c->stream

// nls[k] = byte position of the newline that ends line k (a last line without one ends at nbytes); nls[-1] = (u64)-1 so that line k
// starts at nls[k-1]+1 for every k.  Pool memory: the caller brackets it with a PoolScope.
int build_line_index(harc_amd_ctx *c, const char *d_txt, uint64_t nbytes, const uint64_t **nls_out, uint64_t *total_lines_out, bool *open_tail)
{
    const uint64_t ntiles = (nbytes + NL_TILE - 1) / NL_TILE;
    uint32_t *tilecnt = nullptr; uint64_t *tilebase = nullptr;
    RC_TRY(dalloc(c, &tilecnt, (size_t)ntiles + 1)); RC_TRY(dalloc(c, &tilebase, (size_t)ntiles + 1));
    HIP_TRY(hipMemsetAsync(tilecnt + ntiles, 0, 4, c->stream));
    hipLaunchKernelGGL(k_nl_count, dim3((unsigned)ntiles), dim3(256), 0, c->stream, d_txt, nbytes, tilecnt);
    RC_TRY(prim_excl_scan_u32_to_u64(c, tilecnt, tilebase, (size_t)ntiles + 1));
    uint64_t nlines = 0; char lastch = 0;
    HIP_TRY(hipMemcpyAsync(&nlines, tilebase + ntiles, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&lastch, d_txt + nbytes - 1, 1, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint64_t *nl = nullptr; RC_TRY(dalloc(c, &nl, (size_t)nlines + 8));
    HIP_TRY(hipMemsetAsync(nl, 0xFF, 8, c->stream));
    hipLaunchKernelGGL(k_nl_write, dim3((unsigned)ntiles), dim3(256), 0, c->stream, d_txt, nbytes, (const uint64_t *)tilebase, nl + 1);
    uint64_t total_lines = nlines;
    if (lastch != '\n') {                                         // last line without a newline: it ends at nbytes
        HIP_TRY(hipMemcpyAsync(nl + 1 + nlines, &nbytes, 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        total_lines++;
    }
    *nls_out = nl + 1; *total_lines_out = total_lines;
    if (open_tail) *open_tail = lastch != '\n';
    return HARC_AMD_OK;
}
int text_line_index(harc_amd_ctx *c, const char *d_txt, uint64_t nbytes, const uint64_t **nls, uint64_t *lines, bool *open_tail)
{
    if (nbytes) return build_line_index(c, d_txt, nbytes, nls, lines, open_tail);
    *lines = 0; *open_tail = false;                               // no text, no line; a kernel still reads nls[-1]
    uint64_t *z = nullptr; RC_TRY(dalloc(c, &z, 2));
    HIP_TRY(hipMemsetAsync(z, 0xFF, 16, c->stream));
    *nls = z + 1;
    return HARC_AMD_OK;
}

// the rule kernel over a FASTQ text in device memory, with a line index of its own
extern "C" int harc_amd_third_rule_device(harc_amd_ctx *c, const char *d_fastq, uint64_t n_bytes, uint64_t *n_records, uint32_t *flags_and)
{
    if (!c || !n_records || !flags_and || (n_bytes && !d_fastq)) { harc_set_error("third_rule_device: bad arguments"); return HARC_AMD_EINVAL; }
    *n_records = 0; *flags_and = TH_F_ALL;
    if (n_bytes == 0) return HARC_AMD_OK;
    HIP_TRY(hipSetDevice(c->P.device));
    PoolScope scope(c);
    const uint64_t *nls = nullptr; uint64_t total_lines = 0;
    RC_TRY(build_line_index(c, d_fastq, n_bytes, &nls, &total_lines));
    const uint64_t nrec = (total_lines + 1) / 4;
    unsigned int *d_flags = nullptr; RC_TRY(dalloc(c, &d_flags, 4));
    HIP_TRY(hipMemsetAsync(d_flags, 0xFF, 16, c->stream));
    const bool trace = getenv("HARC_AMD_TRACE") != nullptr;
    double seconds = 0;
    KernelTimer timer(trace ? &seconds : nullptr);
    RC_TRY(timer.begin(c->stream));
    if (nrec) hipLaunchKernelGGL(k_third_rule, G256(nrec * TH_G), (const uint8_t *)d_fastq, nls, nrec, d_flags);
    HIP_TRY(hipGetLastError());
    RC_TRY(timer.end(c->stream));
    unsigned int f = 0;
    HIP_TRY(hipMemcpyAsync(&f, d_flags, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (trace) fprintf(stderr, "[third] device call: %llu records, %llu bytes of text, rule kernel %.3f ms (%.1f GB/s)\n", (unsigned long long)nrec, (unsigned long long)n_bytes,
                       1e3 * seconds, seconds > 0 ? 1e-9 * (double)n_bytes / seconds : 0.0);
    *n_records = nrec; *flags_and = f & TH_F_ALL;
    return HARC_AMD_OK;
}
extern "C" int harc_amd_third_rule_host(const char *fastq, uint64_t n_bytes, uint64_t *n_records, uint32_t *flags_and)
{
    if (!n_records || !flags_and || (n_bytes && !fastq)) { harc_set_error("third_rule_host: bad arguments"); return HARC_AMD_EINVAL; }
    *flags_and = th_text_flags_host((const uint8_t *)fastq, n_bytes, n_records);
    return HARC_AMD_OK;
}
extern "C" int32_t harc_amd_third_rule_of(uint32_t flags_and, uint64_t n_records) { return th_rule_of(flags_and, n_records); }
extern "C" const char *harc_amd_third_rule_name(int32_t rule) { return th_rule_name(rule); }
extern "C" int32_t harc_amd_third_rule_parse(const char *name) { return name ? th_rule_parse(name) : -1; }

// FASTQ text in device memory -> the context's clean reads (2-bit) and N reads (3-bit), a chunk of whole records at a time: a file
// larger than HBM is ingested in pieces (harc_amd_compress_fastq_files_ex), the packed stores grow as the pieces arrive.
struct IngestState {
    uint64_t nC = 0, nN = 0, nrec = 0, nfull = 0;                 // clean reads, reads with N, reads, complete records so far
    std::vector<uint32_t> orderN;                                 // read_order_N.bin: record number of every read with N (preprocess.cpp:102)
    uint64_t total_lines = 0;                                     // the lines the text holds (-q without -p, q_plan: a last record may be cut short)
    // -q without -p on a file that does not stay in HBM (emit_quality_and_ids_streamed): the length of every id line
    bool want_idlen = false;
    std::vector<uint32_t> idlen;
    // -q: the rule of the third lines (third.h), the AND over every piece of every file of the job
    bool want_third = false;
    uint32_t third_and = TH_F_ALL; uint64_t third_n = 0;           // the flags left standing; the records that took part
};
__global__ void k_q_idlen(const uint64_t *nls, uint32_t nid, uint32_t *len)
{
    const uint32_t r = harc_gid32();
    if (r < nid) len[r] = (uint32_t)(nls[4ll * r] - (nls[4ll * r - 1] + 1));
}
static int ingest_begin(harc_amd_ctx *c, IngestState &st)
{
    { const bool w = st.want_idlen, t = st.want_third; st = IngestState(); st.want_idlen = w; st.want_third = t; }
    // same effect as harc_amd_set_reads_* on an empty set: previous inputs and results go
    RC_TRY(harc_amd_set_reads_packed_device(c, nullptr, 0));
    RC_TRY(harc_amd_set_nreads_ascii_device(c, nullptr, 0, (uint32_t)c->P.readlen));
    return HARC_AMD_OK;
}
// grows *b to `need` bytes keeping its first `keep` bytes
static int in_grow(harc_amd_ctx *c, harc_amd_ctx::InBuf *b, size_t need, size_t keep)
{
    if (b->p && b->cap >= need) return HARC_AMD_OK;
    harc_amd_ctx::InBuf nb;
    RC_TRY(harc_in_reserve(c, &nb, need + (keep ? need / 4 : 0)));
    if (keep) HIP_TRY(hipMemcpyAsync(nb.p, b->p, keep, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (b->p) harc_raw_free(c, b->p);
    *b = nb;
    return HARC_AMD_OK;
}
// one chunk of whole 4-line records (the last chunk of the file may end inside a record).  expect_*: the caller's estimate of the final
// counts (0 = unknown), so that the stores are sized once.  whole_records_of (a pair run): the file the chunk comes from; no chunk of it, the last included, may end
// inside a record -- the next file's first line must never be glued to it
static int ingest_append(harc_amd_ctx *c, IngestState &st, const char *d_txt, uint64_t nbytes, bool last, uint64_t expect_clean, uint64_t expect_N, const char *whole_records_of = nullptr)
{
    if (nbytes == 0) return HARC_AMD_OK;
    const int L = c->P.readlen;
    PoolScope scope(c);                                           // scratch goes on every way out
    const uint64_t *nls = nullptr; uint64_t total_lines = 0;
    RC_TRY(build_line_index(c, d_txt, nbytes, &nls, &total_lines));
    if (whole_records_of && (total_lines % 4)) {
        harc_set_error("FASTQ: %s does not hold whole 4-line records (a piece of it ends after line %llu of a record); a pair run does not tolerate a truncated last record", whole_records_of, (unsigned long long)(total_lines % 4));
        return HARC_AMD_EINVAL;
    }
    if (!last && (total_lines % 4)) { harc_set_error("FASTQ: a piece of the file does not hold whole 4-line records (%llu lines)", (unsigned long long)total_lines); return HARC_AMD_EINVAL; }
    // a truncated last record still counts as a read when its sequence line is there: the getline loop handles line 2 before it meets
    // the end of the file (preprocess.cpp:90-111); only `readnum` (case 3, :118) misses it
    const uint64_t nfull = total_lines / 4;
    const uint64_t nrec64 = nfull + ((total_lines % 4) >= 2 ? 1 : 0);
    if (st.nrec + nrec64 > 4294967290ull) { harc_set_error("Too many reads. HARC supports at most 4294967290 reads"); return HARC_AMD_EINVAL; }   // preprocess.cpp:122-126
    const uint32_t nrec = (uint32_t)nrec64;
    uint32_t *isN = nullptr, *isC = nullptr, *rkN = nullptr, *rkC = nullptr; unsigned int *d_err = nullptr;
    RC_TRY(dalloc(c, &isN, (size_t)nrec + 1)); RC_TRY(dalloc(c, &isC, (size_t)nrec + 1)); RC_TRY(dalloc(c, &rkN, (size_t)nrec + 1)); RC_TRY(dalloc(c, &rkC, (size_t)nrec + 1));
    RC_TRY(dalloc(c, &d_err, 4));
    HIP_TRY(hipMemsetAsync(d_err, 0, 16, c->stream));
    HIP_TRY(hipMemsetAsync(isN, 0, ((size_t)nrec + 1) * 4, c->stream)); HIP_TRY(hipMemsetAsync(isC, 0, ((size_t)nrec + 1) * 4, c->stream));
    if (nrec) hipLaunchKernelGGL(k_classify, G256(nrec), d_txt, nls, nrec, L, isN, isC, d_err);
    // -q: the records whose third line is there; their flag word sits behind the error counter and comes back with it
    const uint64_t nthird = st.want_third ? (total_lines + 1) / 4 : 0;
    if (nthird) {
        HIP_TRY(hipMemsetAsync(d_err + 1, 0xFF, 4, c->stream));
        hipLaunchKernelGGL(k_third_rule, G256(nthird * TH_G), (const uint8_t *)d_txt, nls, nthird, d_err + 1);
    }
    RC_TRY(prim_excl_scan_u32(c, isN, rkN, (size_t)nrec + 1)); RC_TRY(prim_excl_scan_u32(c, isC, rkC, (size_t)nrec + 1));
    uint32_t nN = 0, nC = 0; unsigned int errs[2] = { 0, 0 };
    HIP_TRY(hipMemcpyAsync(&nN, rkN + nrec, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&nC, rkC + nrec, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(errs, d_err, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const unsigned int err = errs[0];
    if (nthird) { st.third_and &= errs[1] & TH_F_ALL; st.third_n += nthird; }
    if (err) {
        printf("Read length not fixed. Found reads whose length is not %d\n", L);
        harc_set_error("read length not fixed (%u records differ from %d)", err, L); return HARC_AMD_EINVAL;
    }
    // the packed stores outlive the scratch: raw allocations (as harc_amd_set_reads_*), grown when a piece does not fit
    const uint64_t wantC = std::max<uint64_t>(st.nC + nC, expect_clean), wantN = std::max<uint64_t>(st.nN + nN, expect_N);
    RC_TRY(in_grow(c, &c->own_reads, ((size_t)wantC * c->W + 1) * 8, (size_t)st.nC * c->W * 8));
    RC_TRY(in_grow(c, &c->own_nreads3, ((size_t)wantN * c->W3 + 1) * 8, (size_t)st.nN * c->W3 * 8));
    uint32_t *orderN = nullptr; RC_TRY(dalloc(c, &orderN, (size_t)nN + 1));
    if (nrec) {
        hipLaunchKernelGGL(k_ingest_pack2, G256((uint64_t)nrec * c->W), d_txt, nls, isC, rkC, nrec, L, c->W, (uint64_t *)c->own_reads.p + (size_t)st.nC * c->W);
        hipLaunchKernelGGL(k_ingest_pack3, G256((uint64_t)nrec * c->W3), d_txt, nls, isN, rkN, nrec, L, c->W3, (uint64_t *)c->own_nreads3.p + (size_t)st.nN * c->W3, orderN);
    }
    HIP_TRY(hipGetLastError());
    const size_t at = st.orderN.size();
    st.orderN.resize(at + nN);
    if (nN) HIP_TRY(hipMemcpyAsync(st.orderN.data() + at, orderN, (size_t)nN * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t i = at; i < st.orderN.size(); i++) st.orderN[i] += (uint32_t)st.nrec;       // records of the earlier pieces come first
    if (st.want_idlen) {                                          // one id line per complete record, plus the one of a truncated last record
        const uint32_t nid = (uint32_t)nfull + (total_lines % 4 ? 1u : 0u);
        uint32_t *dl = nullptr; RC_TRY(dalloc(c, &dl, (size_t)nid + 1));
        if (nid) hipLaunchKernelGGL(k_q_idlen, G256(nid), nls, nid, dl);
        const size_t a0 = st.idlen.size();
        st.idlen.resize(a0 + nid);
        if (nid) HIP_TRY(hipMemcpyAsync(st.idlen.data() + a0, dl, (size_t)nid * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    st.total_lines += total_lines;
    st.nC += nC; st.nN += nN; st.nrec += nrec64; st.nfull += nfull;
    return HARC_AMD_OK;
}
static int ingest_finish(harc_amd_ctx *c, IngestState &st)
{
    c->N_own = (uint32_t)st.nC; c->NN_own = (uint32_t)st.nN;
    harc_reset_shard(c);
    c->nrec_own = st.nrec;
    std::vector<uint8_t> &ob = out_buf(c, HARC_AMD_IN_ORDER_N, 0);
    ob.resize(st.orderN.size() * 4);
    if (!st.orderN.empty()) memcpy(ob.data(), st.orderN.data(), ob.size());
    return HARC_AMD_OK;
}

// the whole FASTQ text at once; the original indices of the N reads (read_order_N.bin, u32 each) are returned through
// harc_amd_get_stream(HARC_AMD_IN_ORDER_N)
extern "C" int harc_amd_set_fastq_device(harc_amd_ctx *c, const char *d_txt, uint64_t nbytes, uint64_t *n_records_out)
{
    if (!c || (nbytes && !d_txt)) return HARC_AMD_EINVAL;
    HIP_TRY(hipSetDevice(c->P.device));
    IngestState st;
    RC_TRY(ingest_begin(c, st));
    RC_TRY(ingest_append(c, st, d_txt, nbytes, true, 0, 0));
    RC_TRY(ingest_finish(c, st));
    if (n_records_out) *n_records_out = st.nfull;                 // what preprocess.cpp:134 prints: complete records
    return HARC_AMD_OK;
}


// ------------------------------------------------------------------------------------------------ -q: ids and quality values
// preprocess.cpp:61-118 + reorder_quality.cpp as gathers over the line index.  `rec[p]` names the record whose
// line `k` (0 = id, 3 = quality) becomes output line p.
// the N flags of k_classify again, from read_order_N.bin
__global__ void k_q_scatter_flag(const uint32_t *idx, uint32_t n, uint32_t lim, uint32_t *flag, unsigned int *err)
{
    const uint32_t i = harc_gid32();
    if (i >= n) return;
    const uint32_t r = idx[i];
    if (r >= lim) { atomicAdd(err, 1u); return; }
    flag[r] = 1u;
}
__global__ void k_q_not(const uint32_t *isN, uint32_t n, uint32_t *isC) { const uint32_t r = harc_gid32(); if (r < n) isC[r] = isN[r] ? 0u : 1u; }
__global__ void k_q_idflags(const uint32_t *isN, uint32_t nid, uint32_t *idC, uint32_t *idN)
{
    const uint32_t r = harc_gid32();
    if (r >= nid) return;
    const uint32_t prevN = r ? isN[r - 1] : 0u;                    // preprocess.cpp:83-88 runs before :98-110 of the same record
    idC[r] = prevN ? 0u : 1u; idN[r] = prevN;
}
__global__ void k_q_compact(const uint32_t *flag, const uint32_t *rank, uint32_t n, uint32_t *out)
{
    const uint32_t r = harc_gid32();
    if (r < n && flag[r]) out[rank[r]] = r;
}
__global__ void k_q_gather(const uint32_t *src, uint32_t nsrc, const uint32_t *order, uint32_t n, uint32_t *out, unsigned int *err)
{
    const uint32_t p = harc_gid32();
    if (p >= n) return;
    const uint32_t o = order[p];
    if (o >= nsrc) { atomicAdd(err, 1u); out[p] = 0; return; }
    out[p] = src[o];
}
__global__ void k_q_iota(uint32_t *out, uint32_t n) { const uint32_t p = harc_gid32(); if (p < n) out[p] = p; }
__global__ void k_q_linelen(const uint64_t *nls, const uint32_t *rec, uint32_t n, int k, int want, uint32_t *len, unsigned int *err)
{
    const uint32_t p = harc_gid32();
    if (p >= n) return;
    const int64_t li = 4ll * rec[p] + k;
    const uint64_t l = nls[li] - (nls[li - 1] + 1);
    if (want >= 0 && l != (uint64_t)want) atomicAdd(err, 1u);      // reorder_quality.cpp:78-79 reads quality values at a (readlen+1) stride
    len[p] = (uint32_t)l + 1;
}
// one wave per output line
__global__ __launch_bounds__(256) void k_q_copy(const char *txt, const uint64_t *nls, const uint32_t *rec, const uint64_t *off, uint32_t n, int k, char *out)
{
    const uint32_t p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n) return;
    const int lane = threadIdx.x & 63;
    const int64_t li = 4ll * rec[p] + k;
    const uint64_t s = nls[li - 1] + 1, l = nls[li] - s;
    char *o = out + off[p];
    for (uint64_t j = lane; j < l; j += 64) o[j] = txt[s + j];
    if (lane == 0) o[l] = '\n';
}

// device memory -> an open file, behind what is on the stream
static int write_device_range(harc_amd_ctx *c, const char *d, size_t n, FILE *fo)
{
    std::vector<uint8_t> host;
    const size_t CH = (size_t)256 << 20;
    for (size_t at = 0; at < n; at += CH) {
        const size_t m = n - at < CH ? n - at : CH;
        RC_TRY(harc_d2h(c, host, d + at, m));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (fwrite(host.data(), 1, m, fo) != m) { harc_set_error("short write"); return HARC_AMD_EIO; }
    }
    return HARC_AMD_OK;
}

static int emit_lines(harc_amd_ctx *c, const char *d_txt, const uint64_t *nls, const uint32_t *rec, uint64_t n, int k, int want, FILE *fo)
{
    const uint32_t CH = 1u << 23;
    unsigned int *d_err = nullptr; RC_TRY(dalloc(c, &d_err, 4));
    HIP_TRY(hipMemsetAsync(d_err, 0, 16, c->stream));
    for (uint64_t at = 0; at < n; at += CH) {
        PoolScope scope(c);
        const uint32_t m = (uint32_t)(n - at < CH ? n - at : CH);
        uint32_t *len = nullptr; uint64_t *off = nullptr;
        RC_TRY(dalloc(c, &len, (size_t)m + 1)); RC_TRY(dalloc(c, &off, (size_t)m + 1));
        HIP_TRY(hipMemsetAsync(len + m, 0, 4, c->stream));
        hipLaunchKernelGGL(k_q_linelen, G256(m), nls, rec + at, m, k, want, len, d_err);
        RC_TRY(prim_excl_scan_u32_to_u64(c, len, off, (size_t)m + 1));
        uint64_t total = 0; unsigned int err = 0;
        HIP_TRY(hipMemcpyAsync(&total, off + m, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (err) { harc_set_error("-q without -p needs quality lines of exactly readlen characters (%u differ)", err); return HARC_AMD_EINVAL; }
        char *out = nullptr; RC_TRY(dalloc(c, &out, (size_t)total + 16));
        hipLaunchKernelGGL(k_q_copy, dim3((m + 3) / 4), dim3(256), 0, c->stream, d_txt, nls, rec + at, (const uint64_t *)off, m, k, out);
        RC_TRY(write_device_range(c, out, (size_t)total, fo));
    }
    return HARC_AMD_OK;
}

// -q -p (preprocess.cpp:64-69): quality values and ids in file order; one piece of whole records at a time, appended to the open files
static int emit_q_fileorder(harc_amd_ctx *c, const char *d_txt, uint64_t nbytes, FILE *fq, FILE *fi)
{
    if (nbytes == 0) return HARC_AMD_OK;
    PoolScope scope(c);
    const uint64_t *nls = nullptr; uint64_t total_lines = 0;
    RC_TRY(build_line_index(c, d_txt, nbytes, &nls, &total_lines));
    const uint32_t nrec = (uint32_t)(total_lines / 4);
    const uint32_t nid = nrec + (total_lines % 4 ? 1u : 0u);       // the id line of a truncated last record is still written (case 0 of the getline loop)
    uint32_t *rec = nullptr; RC_TRY(dalloc(c, &rec, (size_t)nid + 1));
    hipLaunchKernelGGL(k_q_iota, G256((size_t)nid + 1), rec, nid + 1);
    RC_TRY(emit_lines(c, d_txt, nls, rec, nrec, 3, -1, fq));
    RC_TRY(emit_lines(c, d_txt, nls, rec, nid, 0, -1, fi));
    return HARC_AMD_OK;
}

// Which record's quality line / id line becomes output line p (reorder_quality.cpp:47-133, :140-208), from the per-record flags: qrec[nC + nN],
// irec[nC + nidN].  Pool memory of the caller's bracket.
static int q_routes(harc_amd_ctx *c, const uint32_t *isN, const uint32_t *isC, uint32_t nrec, uint32_t nid, unsigned int *d_err, uint32_t **qrec_out, uint32_t **irec_out, uint32_t *nidN_out)
{
    const void *ho = nullptr, *hn = nullptr; size_t ho_len = 0, hn_len = 0;
    RC_TRY(harc_amd_get_stream(c, HARC_AMD_S2_ORDER, 0, &ho, &ho_len)); RC_TRY(harc_amd_get_stream(c, HARC_AMD_S2_ORDER_N_PE, 0, &hn, &hn_len));
    const uint32_t nC = c->N, nN = c->NN;
    if (ho_len != (size_t)nC * 4 || hn_len != (size_t)nN * 4) { harc_set_error("-q: order streams do not match the read counts"); return HARC_AMD_ESTATE; }
    uint32_t *rk, *idC, *idN, *cleanrec, *nrecs, *idcrec, *idnrec, *d_ord, *d_ordn, *qrec, *irec;
    RC_TRY(dalloc(c, &rk, (size_t)nid + 2));
    RC_TRY(dalloc(c, &idC, (size_t)nid + 1)); RC_TRY(dalloc(c, &idN, (size_t)nid + 1));
    RC_TRY(dalloc(c, &cleanrec, (size_t)nC + 1)); RC_TRY(dalloc(c, &nrecs, (size_t)nN + 1)); RC_TRY(dalloc(c, &idcrec, (size_t)nid + 1)); RC_TRY(dalloc(c, &idnrec, (size_t)nid + 1));
    RC_TRY(dalloc(c, &d_ord, (size_t)nC + 1)); RC_TRY(dalloc(c, &d_ordn, (size_t)nN + 1)); RC_TRY(dalloc(c, &qrec, (size_t)nC + nN + 1)); RC_TRY(dalloc(c, &irec, (size_t)nC + nid + 1));
    if (nC) HIP_TRY(hipMemcpyAsync(d_ord, ho, ho_len, hipMemcpyHostToDevice, c->stream));
    if (nN) HIP_TRY(hipMemcpyAsync(d_ordn, hn, hn_len, hipMemcpyHostToDevice, c->stream));
    // quality: clean records gathered by read_order.bin, then N records gathered by read_order_N_pe.bin (reorder_quality.cpp:47-133)
    RC_TRY(prim_excl_scan_u32(c, isC, rk, (size_t)nrec + 1));
    if (nrec) hipLaunchKernelGGL(k_q_compact, G256(nrec), isC, rk, nrec, cleanrec);
    RC_TRY(prim_excl_scan_u32(c, isN, rk, (size_t)nrec + 1));
    if (nrec) hipLaunchKernelGGL(k_q_compact, G256(nrec), isN, rk, nrec, nrecs);
    if (nC) hipLaunchKernelGGL(k_q_gather, G256(nC), cleanrec, nC, d_ord, nC, qrec, d_err);
    if (nN) hipLaunchKernelGGL(k_q_gather, G256(nN), nrecs, nN, d_ordn, nN, qrec + nC, d_err);
    // ids: routed by the PREVIOUS record's N flag; the clean list gathered by read_order.bin, the N list appended as it is
    // (reorder_id_N writes its result over input_N.quality, reorder_quality.cpp:208, so reorder_id appends input_N.id untouched, :181)
    uint32_t nidC = 0, nidN = 0;
    if (nid) {
        hipLaunchKernelGGL(k_q_idflags, G256(nid), isN, nid, idC, idN);
        HIP_TRY(hipMemsetAsync(idC + nid, 0, 4, c->stream)); HIP_TRY(hipMemsetAsync(idN + nid, 0, 4, c->stream));
        RC_TRY(prim_excl_scan_u32(c, idC, rk, (size_t)nid + 1));
        hipLaunchKernelGGL(k_q_compact, G256(nid), idC, rk, nid, idcrec);
        HIP_TRY(hipMemcpyAsync(&nidC, rk + nid, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        RC_TRY(prim_excl_scan_u32(c, idN, rk, (size_t)nid + 1));
        hipLaunchKernelGGL(k_q_compact, G256(nid), idN, rk, nid, idnrec);
        nidN = nid - nidC;
    }
    if (nC) hipLaunchKernelGGL(k_q_gather, G256(nC), idcrec, nidC, d_ord, nC, irec, d_err);
    if (nidN) HIP_TRY(hipMemcpyAsync(irec + nC, idnrec, (size_t)nidN * 4, hipMemcpyDeviceToDevice, c->stream));
    unsigned int err = 0;
    HIP_TRY(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (err) { harc_set_error("-q: order files and FASTQ disagree (%u entries)", err); return HARC_AMD_ESTATE; }
    *qrec_out = qrec; *irec_out = irec; *nidN_out = nidN;
    return HARC_AMD_OK;
}

// output.quality and output.id of an archive, or the quality / id parts of a rank: both are there or the call fails, both are closed on every way out
struct QIdFiles {
    FILE *fq = nullptr, *fi = nullptr, *fi2 = nullptr;             // fi2: output.id2, the ids of the second file of a pair run
    ~QIdFiles() { if (fq) fclose(fq); if (fi) fclose(fi); if (fi2) fclose(fi2); }
    bool open2(const std::string &q, const std::string &i) { fq = fopen(q.c_str(), "wb"); fi = fopen(i.c_str(), "wb"); return fq && fi; }
    int open(const std::string &od)
    {
        if (open2(od + "output.quality", od + "output.id")) return HARC_AMD_OK;
        harc_set_error("cannot create %soutput.quality / output.id", od.c_str()); return HARC_AMD_EIO;
    }
    int open_pair(const std::string &od)
    {
        RC_TRY(open(od));
        fi2 = fopen((od + "output.id2").c_str(), "wb");
        if (fi2) return HARC_AMD_OK;
        harc_set_error("cannot create %soutput.id2", od.c_str()); return HARC_AMD_EIO;
    }
    int open_parts(const std::string &sd, const std::string &r)
    {
        if (open2(sd + "quality" + r, sd + "id" + r)) return HARC_AMD_OK;
        harc_set_error("cannot create the quality / id parts under %s", sd.c_str()); return HARC_AMD_EIO;
    }
};

// -q without -p, what the walk over the resident text and the walk over the streamed file share: the refusal of a truncated last record, the counts, the
// per-record flags (from read_order_N.bin as the ingest kept it) and the routes.  Pool memory of the caller's bracket.
struct QPlan { uint32_t nrec = 0, nid = 0, nidN = 0; uint32_t *qrec = nullptr, *irec = nullptr; unsigned int *d_err = nullptr; };     // d_err: zero on return
static int q_plan(harc_amd_ctx *c, const IngestState &st, QPlan *q)
{
    if ((st.total_lines % 4) >= 2) {                              // that read has no quality line: reorder_quality.cpp would walk off its arrays
        harc_set_error("-q without -p: the last FASTQ record is truncated (its read is kept, its quality line is missing)"); return HARC_AMD_EINVAL;
    }
    const uint32_t nrec = (uint32_t)st.nfull;
    const uint32_t nid = nrec + (st.total_lines % 4 ? 1u : 0u);    // the id line of a truncated last record is still written (case 0 of the getline loop)
    uint32_t *isN, *isC;
    RC_TRY(dalloc(c, &isN, (size_t)nid + 1)); RC_TRY(dalloc(c, &isC, (size_t)nid + 1)); RC_TRY(dalloc(c, &q->d_err, 4));
    HIP_TRY(hipMemsetAsync(q->d_err, 0, 16, c->stream));
    HIP_TRY(hipMemsetAsync(isN, 0, ((size_t)nid + 1) * 4, c->stream)); HIP_TRY(hipMemsetAsync(isC, 0, ((size_t)nid + 1) * 4, c->stream));
    {
        PoolScope tmp(c);
        const uint32_t nN = (uint32_t)st.orderN.size();
        uint32_t *d_on = nullptr; RC_TRY(dalloc(c, &d_on, (size_t)nN + 1));
        if (nN) { HIP_TRY(hipMemcpyAsync(d_on, st.orderN.data(), (size_t)nN * 4, hipMemcpyHostToDevice, c->stream)); hipLaunchKernelGGL(k_q_scatter_flag, G256(nN), d_on, nN, nrec, isN, q->d_err); }
        if (nrec) hipLaunchKernelGGL(k_q_not, G256(nrec), isN, nrec, isC);
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    q->nrec = nrec; q->nid = nid;
    return q_routes(c, isN, isC, nrec, nid, q->d_err, &q->qrec, &q->irec, &q->nidN);
}

// the text is resident: the line index of the whole text, the output lines gathered through it
static int emit_quality_and_ids(harc_amd_ctx *c, const char *d_txt, uint64_t nbytes, const IngestState &st, const std::string &od)
{
    QIdFiles out; RC_TRY(out.open(od));
    if (nbytes == 0) return HARC_AMD_OK;
    PoolScope scope(c);
    QPlan q; RC_TRY(q_plan(c, st, &q));
    const uint64_t *nls = nullptr; uint64_t total_lines = 0;
    RC_TRY(build_line_index(c, d_txt, nbytes, &nls, &total_lines));
    RC_TRY(emit_lines(c, d_txt, nls, q.qrec, (uint64_t)c->N + c->NN, 3, c->P.readlen, out.fq));
    RC_TRY(emit_lines(c, d_txt, nls, q.irec, (uint64_t)c->N + q.nidN, 0, -1, out.fi));
    return HARC_AMD_OK;
}

// ---- -q without -p when the FASTQ text does not stay in HBM: the reference permutes quality values and ids in 4-8 bins of host memory, reading
// the files once per bin (reorder_quality.cpp:61-77).  Here: the routes (which record's line becomes output line p) come from the per-record N
// flags and the id-line lengths kept by the ingest; the OUTPUT is cut into bins that fit HBM, and for every bin the FASTQ file is streamed
// through the GPU once more, piece by piece, every line that belongs to the bin copied to its place (quality lines have a fixed stride -- they
// must be readlen long, reorder_quality.cpp:78-79 -- id lines go by a prefix sum of their lengths).  Quality and id bins share a pass.
__global__ void k_q_invert(const uint32_t *rec, uint32_t n, uint32_t *pos) { const uint32_t p = harc_gid32(); if (p < n) pos[rec[p]] = p; }
__global__ void k_q_outlen(const uint32_t *idlen, const uint32_t *rec, uint32_t n, uint32_t *len) { const uint32_t p = harc_gid32(); if (p < n) len[p] = idlen[rec[p]] + 1u; }
// first p in [lo, n] with off[p] - off[lo] > budget, minus one (at least lo + 1 when lo < n): the end of the bin that starts at lo
__global__ void k_q_bin_end(const uint64_t *off, uint32_t lo, uint32_t n, uint64_t budget, uint32_t *out)
{
    if (blockIdx.x || threadIdx.x) return;
    const uint64_t base = off[lo];
    uint32_t a = lo, b = n;                                       // largest p with off[p] - base <= budget
    while (a < b) { const uint32_t mid = a + (b - a + 1) / 2; if (off[mid] - base <= budget) a = mid; else b = mid - 1; }
    if (a == lo && lo < n) a = lo + 1;                            // a single line longer than the budget still goes out
    out[0] = a;
}
// one wave per record of the piece: its quality line and its id line, each if its output line lies in the bin being filled
__global__ __launch_bounds__(256) void k_q_place(const char *txt, const uint64_t *nls, uint32_t nrec, uint32_t nid, uint32_t base, int L,
                                                 const uint32_t *posQ, uint32_t q0, uint32_t q1, char *outQ,
                                                 const uint32_t *posI, const uint64_t *offI, uint32_t i0, uint32_t i1, char *outI, unsigned int *err)
{
    const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r < nrec) {
        const uint32_t p = posQ[base + r];
        if (p >= q0 && p < q1) {
            const uint64_t s = nls[4ll * r + 2] + 1, l = nls[4ll * r + 3] - s;
            if (l != (uint64_t)L) { if (lane == 0) atomicAdd(err, 1u); }
            else {
                char *o = outQ + (size_t)(p - q0) * (size_t)(L + 1);
                for (uint64_t j = lane; j < l; j += 64) o[j] = txt[s + j];
                if (lane == 0) o[l] = '\n';
            }
        }
    }
    if (r < nid) {
        const uint32_t p = posI[base + r];
        if (p >= i0 && p < i1) {
            const uint64_t s = nls[4ll * r - 1] + 1, l = nls[4ll * r] - s;
            char *o = outI + (offI[p] - offI[i0]);
            for (uint64_t j = lane; j < l; j += 64) o[j] = txt[s + j];
            if (lane == 0) o[l] = '\n';
        }
    }
}
static int record_start_at_or_after(FILE *f, uint64_t pos, uint64_t fsz, uint64_t *out);
template <class F> static int text_pieces(harc_amd_ctx *c, FILE *f, const char *name, uint64_t lo, uint64_t end, uint64_t fsz, bool bgzf,
                                          double *t_wait, double *t_inflate, F &&fn);
// bytes of the file per piece of the ingest: 1 GiB of FASTQ; 4 GiB of BGZF (compressed bytes), because the inflate kernel runs one lane per
// member and a piece of 1 GiB holds ~27 000 of them, too few to fill the chip (NOTES.md, BGZF); HARC_AMD_INGEST_CHUNK in tests (pieces of a few records)
static uint64_t ingest_piece_bytes(bool bgzf)
{
    const uint64_t piece = env_u64("HARC_AMD_INGEST_CHUNK", (uint64_t)1 << (bgzf ? 32 : 30));
    return piece < 16 ? 16 : piece;
}
static int emit_quality_and_ids_streamed(harc_amd_ctx *c, FILE *f, const char *name, uint64_t fsz, bool bgzf, const IngestState &st, const std::string &od)
{
    QIdFiles out; RC_TRY(out.open(od));
    if (fsz == 0) return HARC_AMD_OK;
    const int L = c->P.readlen;
    PoolScope scope(c);
    QPlan q; RC_TRY(q_plan(c, st, &q));
    const uint32_t nrec = q.nrec, nid = q.nid, nidN = q.nidN, *qrec = q.qrec, *irec = q.irec; unsigned int *d_err = q.d_err;
    if (st.idlen.size() != (size_t)nid) { harc_set_error("-q: %zu id lines recorded, %u expected", st.idlen.size(), nid); return HARC_AMD_EINTERNAL; }
    const uint32_t nC = c->N, nN = c->NN, nQ = nC + nN, nI = nC + nidN;
    uint32_t *posQ, *posI, *d_idlen, *lenI, *d_end; uint64_t *offI;
    RC_TRY(dalloc(c, &posQ, (size_t)nrec + 1)); RC_TRY(dalloc(c, &posI, (size_t)nid + 1)); RC_TRY(dalloc(c, &d_idlen, (size_t)nid + 1));
    RC_TRY(dalloc(c, &lenI, (size_t)nI + 1)); RC_TRY(dalloc(c, &offI, (size_t)nI + 1)); RC_TRY(dalloc(c, &d_end, 4));
    HIP_TRY(hipMemsetAsync(posQ, 0xFF, ((size_t)nrec + 1) * 4, c->stream)); HIP_TRY(hipMemsetAsync(posI, 0xFF, ((size_t)nid + 1) * 4, c->stream));
    if (nQ) hipLaunchKernelGGL(k_q_invert, G256(nQ), qrec, nQ, posQ);
    if (nI) hipLaunchKernelGGL(k_q_invert, G256(nI), irec, nI, posI);
    if (nid) HIP_TRY(hipMemcpyAsync(d_idlen, st.idlen.data(), (size_t)nid * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(lenI + nI, 0, 4, c->stream));
    if (nI) hipLaunchKernelGGL(k_q_outlen, G256(nI), d_idlen, irec, nI, lenI);
    RC_TRY(prim_excl_scan_u32_to_u64(c, lenI, offI, (size_t)nI + 1));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // bytes of output one pass holds, per file
    size_t budget;
    {
        size_t fr = 0, tot = 0; (void)hipMemGetInfo(&fr, &tot);
        budget = (size_t)(0.25 * (double)fr);
        if (budget > ((size_t)32 << 30)) budget = (size_t)32 << 30;
        if (budget < ((size_t)64 << 20)) budget = (size_t)64 << 20;
        budget = (size_t)env_u64("HARC_AMD_Q_BIN", budget);        // tests: bins of a few lines
    }
    uint32_t q0 = 0, i0 = 0; int passes = 0;
    while (q0 < nQ || i0 < nI) {
        PoolScope pass_scope(c);
        uint64_t perq = budget / (uint64_t)(L + 1); if (perq < 1) perq = 1;
        const uint32_t q1 = (uint64_t)nQ - q0 > perq ? q0 + (uint32_t)perq : nQ;
        uint32_t i1 = i0;
        uint64_t ob[2] = { 0, 0 };
        if (i0 < nI) {
            hipLaunchKernelGGL(k_q_bin_end, dim3(1), dim3(1), 0, c->stream, (const uint64_t *)offI, i0, nI, (uint64_t)budget, d_end);
            HIP_TRY(hipMemcpyAsync(&i1, d_end, 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            HIP_TRY(hipMemcpyAsync(&ob[0], offI + i0, 8, hipMemcpyDeviceToHost, c->stream)); HIP_TRY(hipMemcpyAsync(&ob[1], offI + i1, 8, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        const size_t bytesQ = (size_t)(q1 - q0) * (size_t)(L + 1), bytesI = (size_t)(ob[1] - ob[0]);
        char *outQ = nullptr, *outI = nullptr;
        RC_TRY(dalloc(c, &outQ, bytesQ + 16)); RC_TRY(dalloc(c, &outI, bytesI + 16));
        uint32_t base = 0;
        RC_TRY(text_pieces(c, f, name, 0, fsz, fsz, bgzf, nullptr, nullptr, [&](const char *d_txt, uint64_t n, bool, uint64_t) -> int {
            if (n == 0) return HARC_AMD_OK;
            PoolScope piece_scope(c);
            const uint64_t *nls = nullptr; uint64_t tl = 0;
            RC_TRY(build_line_index(c, d_txt, n, &nls, &tl));
            const uint32_t pr = (uint32_t)(tl / 4), pi = pr + (tl % 4 ? 1u : 0u);
            if ((uint64_t)base + pi > (uint64_t)nid) { harc_set_error("-q: the FASTQ file changed between the passes"); return HARC_AMD_EIO; }
            if (pi) hipLaunchKernelGGL(k_q_place, dim3((pi + 3) / 4), dim3(256), 0, c->stream, d_txt, nls, pr, pi, base, L, (const uint32_t *)posQ, q0, q1, outQ,
                                       (const uint32_t *)posI, (const uint64_t *)offI, i0, i1, outI, d_err);
            HIP_TRY(hipStreamSynchronize(c->stream));
            base += pr;
            return HARC_AMD_OK;
        }));
        unsigned int err = 0;
        HIP_TRY(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (err) { harc_set_error("-q without -p needs quality lines of exactly readlen characters (%u differ)", err); return HARC_AMD_EINVAL; }
        RC_TRY(write_device_range(c, outQ, bytesQ, out.fq)); RC_TRY(write_device_range(c, outI, bytesI, out.fi));
        q0 = q1; i0 = i1; passes++;
    }
    if (getenv("HARC_AMD_TRACE")) fprintf(stderr, "[-q] quality values and ids permuted in %d passes over the FASTQ file (%zu bytes of each per pass)\n", passes, budget);
    return HARC_AMD_OK;
}

// ------------------------------------------------------------------------------------------------ file drivers
// Where the wall time of the last harc_amd_compress_fastq_files_ex of this process went (seconds; harc_amd_last_fastq_timing): [0] context + device pool,
// [1] ingest = file -> HBM -> packed stores, reads / uploads / kernels overlapped, [2] of it the calling thread waiting for the reader threads (file-read bound),
// [3] of it the device's line index / classify / pack kernels and their syncs, [4] reorder, [5] encode (the D2H of the streams inside), [6] stream files written,
// [7] total, [8] of [1] the BGZF member scan and inflate (0 for a plain file)
static double g_fastq_timing[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
extern "C" int harc_amd_last_fastq_timing(double *out, int32_t n)
{
    if (!out || n < 1) return HARC_AMD_EINVAL;
    for (int i = 0; i < n; i++) out[i] = i < 9 ? g_fastq_timing[i] : 0.0;
    return HARC_AMD_OK;
}
// bytes [lo, hi) of the file -> device memory
static int load_file_range(harc_amd_ctx *c, const char *name, uint64_t lo, uint64_t hi, DevBuf *b)
{
    const uint64_t n = hi - lo;
    RC_TRY(dev_reserve(b, (size_t)n));
    if (n) {
        FileFeeder fd(c, name);
        RC_TRY(fd.start({ { lo, hi } }));
        RC_TRY(fd.upload_piece(0, b->p, nullptr));
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) { harc_set_error("upload of %s failed", name); return HARC_AMD_ENODEVICE; }
    return HARC_AMD_OK;
}
// the FASTQ input of a file-level call: open for the looks at the record boundaries (record_start_at_or_after), its size, closed on every way out
struct InFile {
    FILE *f = nullptr; uint64_t size = 0;
    ~InFile() { if (f) fclose(f); }
    int open(const char *path)
    {
        f = fopen(path, "rb");
        if (!f) { harc_set_error("cannot open %s", path); return HARC_AMD_EIO; }
        fseeko(f, 0, SEEK_END); size = (uint64_t)ftello(f);
        return HARC_AMD_OK;
    }
};

// first byte >= pos at which a FASTQ record starts: a line that begins with '@' whose second successor begins with '+'.  (A quality
// line may begin with '@' too, but then the line two further on is a sequence line, which never begins with '+'.)
static int record_start_at_or_after(FILE *f, uint64_t pos, uint64_t fsz, uint64_t *out)
{
    if (pos == 0) { *out = 0; return HARC_AMD_OK; }
    if (pos >= fsz) { *out = fsz; return HARC_AMD_OK; }
    std::vector<char> buf;
    for (size_t win = (size_t)1 << 16;; win <<= 1) {
        const uint64_t lo = pos - 1;                              // the byte before pos tells whether pos starts a line
        const uint64_t n = fsz - lo < win ? fsz - lo : win;
        buf.resize((size_t)n);
        if (fseeko(f, (off_t)lo, SEEK_SET) != 0 || fread(buf.data(), 1, (size_t)n, f) != (size_t)n) { harc_set_error("cannot read the FASTQ file around byte %llu", (unsigned long long)pos); return HARC_AMD_EIO; }
        std::vector<size_t> ls;                                   // line starts inside the window (offsets into buf)
        for (size_t i = 0; i + 1 < (size_t)n; i++) if (buf[i] == '\n') ls.push_back(i + 1);
        for (size_t k = 0; k + 2 < ls.size(); k++)
            if (buf[ls[k]] == '@' && buf[ls[k + 2]] == '+') { *out = lo + ls[k]; return HARC_AMD_OK; }
        if (lo + n >= fsz) { *out = fsz; return HARC_AMD_OK; }   // no further record
    }
}
// The last record start in d_txt[0 .. n) by the rule of record_start_at_or_after (a line that begins with '@' whose second successor begins with '+'),
// looked for from the end of the text through a window that grows until one is found: what lies before it is whole records (the text starts at a
// record), the rest is carried into the next piece.  0 when no record start is seen but the first.
static int last_record_start(harc_amd_ctx *c, const char *d_txt, uint64_t n, uint64_t *cut)
{
    *cut = 0;
    std::vector<char> buf;
    std::vector<size_t> ls;
    for (uint64_t win = (uint64_t)1 << 16;; win <<= 2) {
        const uint64_t w = std::min<uint64_t>(win, n), lo = n - w;
        if (w == 0) return HARC_AMD_OK;
        buf.resize((size_t)w);
        HIP_TRY(hipMemcpyAsync(buf.data(), d_txt + lo, (size_t)w, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        ls.clear();                                               // line starts inside the window whose first byte is there
        if (lo == 0) ls.push_back(0);
        for (size_t i = 1; i < (size_t)w; i++) if (buf[i - 1] == '\n') ls.push_back(i);
        for (size_t k = ls.size(); k-- > 0;)
            if (k + 2 < ls.size() && buf[ls[k]] == '@' && buf[ls[k + 2]] == '+') { *cut = lo + ls[k]; return HARC_AMD_OK; }
        if (lo == 0) return HARC_AMD_OK;
    }
}
// The text of bytes [lo, end) of the file as pieces of whole 4-line records, in file order -- what ingest_file_range, the in-HBM -q load of a BGZF
// file and emit_quality_and_ids_streamed consume: fn(d_txt, nbytes, last, at) with `at` the file offset the piece came from (a measure of progress).
// Plain FASTQ: byte ranges that end where a record starts (a 64-KB look at the file per boundary), read through the FileFeeder -- the readers run
// ahead over all pieces, two device buffers alternate.  BGZF (whole files only): compressed ranges [a_p, a_p+1 + 64 KiB) through the same feeder;
// piece p owns the members that START in [a_p, a_p+1) (a member is at most 64 KiB, so they are whole), their text is inflated behind the incomplete
// record carried over from piece p - 1 and cut after its last whole record, the rest is carried on.  HARC_AMD_INGEST_CHUNK: file bytes per piece
// (compressed bytes for BGZF; tests: pieces of a few records).  t_wait / t_inflate (may be null): seconds waited for the readers / in the member
// scan and inflate.
template <class F> static int text_pieces(harc_amd_ctx *c, FILE *f, const char *name, uint64_t lo, uint64_t end, uint64_t fsz, bool bgzf,
                                          double *t_wait, double *t_inflate, F &&fn)
{
    const uint64_t piece = ingest_piece_bytes(bgzf);
    LapTimer tm{ "[ingest]" };
    const uint64_t SLOP = 65536;                                  // BGZF: a member is at most BSIZE + 1 = 65536 bytes
    // the pieces first, so that the readers can run ahead over all of them
    std::vector<std::pair<uint64_t, uint64_t>> pieces;            // file ranges that are read
    std::vector<uint64_t> owned;                                  // BGZF: end of the range whose members a piece owns
    uint64_t maxlen = 0;
    if (bgzf) {
        for (uint64_t a = lo; a < end; a += piece) {
            const uint64_t oe = end - a > piece ? a + piece : end;
            pieces.emplace_back(a, std::min<uint64_t>(end, oe + SLOP)); owned.push_back(oe);
            maxlen = std::max<uint64_t>(maxlen, pieces.back().second - a);
        }
    } else {
        for (uint64_t a = lo; a < end;) {
            uint64_t hi = end;
            if (end - a > piece) { RC_TRY(record_start_at_or_after(f, a + piece, fsz, &hi)); if (hi > end) hi = end; if (hi <= a) hi = end; }
            pieces.emplace_back(a, hi); if (hi - a > maxlen) maxlen = hi - a;
            a = hi;
        }
    }
    if (pieces.empty()) return HARC_AMD_OK;
    tm.lap("piece boundaries");
    // two device buffers: piece i + 1 is uploaded (behind piece i's kernels on the stream) while the host still waits for piece i's counts
    DevBuf db[4] = { { c }, { c }, { c }, { c } };                // BGZF: the text buffers db[2 + (p & 1)], grown as needed
    RC_TRY(dev_reserve(&db[0], (size_t)maxlen));
    if (pieces.size() > 1) RC_TRY(dev_reserve(&db[1], (size_t)maxlen));
    tm.lap("two device buffers");
    FileFeeder feed(c, name);
    RC_TRY(feed.start(pieces));
    tm.lap("feeder started (file mapped, ring pinned, readers running)");
    uint64_t next = lo, carry = 0; const char *carry_at = nullptr;   // BGZF: where the next member starts; the text carried into the next piece
    for (size_t p = 0; p < pieces.size(); p++) {
        const uint64_t a = pieces[p].first, hi = pieces[p].second;
        char *d_in = db[p & 1].p;
        const double tu = mono_now();
        RC_TRY(feed.upload_piece(p, d_in, p + 1 < pieces.size() ? db[(p + 1) & 1].p : nullptr));
        if (t_wait) *t_wait += mono_now() - tu;
        if (!bgzf) { RC_TRY(fn((const char *)d_in, hi - a, hi == fsz, a)); continue; }
        const double ti = mono_now();
        BgzfPlan plan;
        RC_TRY(harc_bgzf_plan(c, (const uint8_t *)d_in, hi - a, next - a, owned[p] - a, a, &plan));
        const size_t need = (size_t)(carry + plan.text);
        DevBuf &tbuf = db[2 + (p & 1)];
        if (!tbuf.p || tbuf.cap < need) RC_TRY(dev_reserve(&tbuf, need + need / 4));   // a quarter of headroom: a slightly longer piece does not reallocate
        char *const tb = tbuf.p;
        if (carry) HIP_TRY(hipMemcpyAsync(tb, carry_at, (size_t)carry, hipMemcpyDeviceToDevice, c->stream));
        RC_TRY(harc_bgzf_run(c, (const uint8_t *)d_in, plan, a, tb + carry));
        if (t_inflate) *t_inflate += mono_now() - ti;
        next = a + plan.next;
        const uint64_t total = carry + plan.text;
        if (p + 1 == pieces.size()) {                             // a last piece may hold no text at all (bgzip's EOF marker alone)
            if (total) RC_TRY(fn((const char *)tb, total, true, a));
            break;
        }
        uint64_t cut = 0;
        RC_TRY(last_record_start(c, tb, total, &cut));
        if (cut) RC_TRY(fn((const char *)tb, cut, false, a));
        carry = total - cut; carry_at = tb + cut;
    }
    tm.lap("pieces uploaded and processed");
    return HARC_AMD_OK;
}
// The records of bytes [lo, end) of the file, a piece at a time: every piece goes to HBM, is indexed, classified and packed, then makes room
// for the next -- the file never has to fit next to the dictionaries.  With fq / fi (-q -p) the quality and id lines of every piece
// are written out in file order on the way.
static int ingest_file_range(harc_amd_ctx *c, FILE *f, const char *name, uint64_t lo, uint64_t end, uint64_t fsz, bool bgzf, IngestState &st, FILE *fq, FILE *fi)
{
    RC_TRY(ingest_begin(c, st));
    const uint64_t start = lo;
    RC_TRY(text_pieces(c, f, name, lo, end, fsz, bgzf, &g_fastq_timing[2], &g_fastq_timing[8], [&](const char *d_txt, uint64_t n, bool last, uint64_t a) -> int {
        const double ta = mono_now();
        // the first piece tells how many reads the whole range will hold, give or take: the stores are sized once
        uint64_t expC = 0, expN = 0;
        if (a > start) { const double scale = 1.03 * (double)(end - start) / (double)(a - start); expC = (uint64_t)(scale * (double)st.nC); expN = (uint64_t)(scale * (double)st.nN); }
        RC_TRY(ingest_append(c, st, d_txt, n, last, expC, expN));
        g_fastq_timing[3] += mono_now() - ta;
        if (fq) RC_TRY(emit_q_fileorder(c, d_txt, n, fq, fi));
        return HARC_AMD_OK;
    }));
    return ingest_finish(c, st);
}
// The records of two files as ONE job (./harc -c R1 -2 R2 -p): the pieces of file 1, then the pieces of file 2, into the same IngestState, so that read_order_N.bin,
// the record numbers and the packed stores continue across the boundary; each file is plain or BGZF on its own.  Neither file may end inside a record or without
// its last newline.  With fq (-q): output.quality takes the lines of both files in order, fi the ids of file 1 and fi2 those of file 2.  nrec[k]: records of file k
static int ingest_file_pair(harc_amd_ctx *c, FILE *const f[2], const char *const name[2], const uint64_t fsz[2], const bool bgzf[2], IngestState &st, FILE *fq, FILE *fi, FILE *fi2,
                            uint64_t nrec[2])
{
    RC_TRY(ingest_begin(c, st));
    for (int k = 0; k < 2; k++) {
        const uint64_t before = st.nfull;
        RC_TRY(text_pieces(c, f[k], name[k], 0, fsz[k], fsz[k], bgzf[k], &g_fastq_timing[2], &g_fastq_timing[8], [&](const char *d_txt, uint64_t n, bool last, uint64_t a) -> int {
            const double ta = mono_now();
            // the two files hold the same number of records: file k is done to the fraction a / fsz[k], the job to (k + that) / 2; the stores are sized once
            uint64_t expC = 0, expN = 0;
            const double frac = 0.5 * ((double)k + (double)a / (double)fsz[k]);
            if (frac > 0) { expC = (uint64_t)(1.03 * (double)st.nC / frac); expN = (uint64_t)(1.03 * (double)st.nN / frac); }
            if (last && n) {
                char lastch = 0;
                HIP_TRY(hipMemcpyAsync(&lastch, d_txt + n - 1, 1, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                if (lastch != '\n') { harc_set_error("FASTQ: %s does not end in a newline; a pair run does not tolerate a last line that is cut short", name[k]); return HARC_AMD_EINVAL; }
            }
            RC_TRY(ingest_append(c, st, d_txt, n, false, expC, expN, name[k]));
            g_fastq_timing[3] += mono_now() - ta;
            if (fq) RC_TRY(emit_q_fileorder(c, d_txt, n, fq, k ? fi2 : fi));
            return HARC_AMD_OK;
        }));
        nrec[k] = st.nfull - before;
    }
    if (nrec[0] != nrec[1]) {
        harc_set_error("the two files of the pair hold different numbers of records: %s %llu, %s %llu; mates are paired by their place", name[0], (unsigned long long)nrec[0], name[1], (unsigned long long)nrec[1]);
        return HARC_AMD_EINVAL;
    }
    return ingest_finish(c, st);
}

// What the first bytes of a file say: 0 = not gzip, 1 = BGZF (the first member carries a BC subfield), -1 = another gzip.  *ratio (may be null):
// text bytes per compressed byte over the members that start in the first MB (the -q mode is chosen by the size of the text).
static int gzip_kind(const char *path, double *ratio)
{
    FILE *f = fopen(path, "rb");
    if (!f) return 0;
    std::vector<uint8_t> b((size_t)1 << 20);
    const size_t got = fread(b.data(), 1, b.size(), f);
    fclose(f);
    if (got < 2 || b[0] != 0x1f || b[1] != 0x8b) return 0;
    uint32_t bs = 0, hdr = 0;
    if (!im_bgzf_header(b.data(), got, &bs, &hdr)) return -1;
    if (ratio) {
        uint64_t pos = 0, txt = 0;
        while (pos < got && im_bgzf_header(b.data() + pos, got - pos, &bs, &hdr) && pos + bs + 1 <= got) { txt += im_le32(b.data() + pos + bs + 1 - 4); pos += (uint64_t)bs + 1; }
        *ratio = pos ? (double)txt / (double)pos : 1.0;
    }
    return 1;
}

// FASTQ file -> every stage-II file under <basedir>/output (+ read_order_N.bin, numreads.bin): harc:50-69 without input_clean.dna
extern "C" int harc_amd_compress_fastq_files_ex(const harc_amd_params *params, const char *fastq, const char *basedir, int32_t preserve_order, int32_t preserve_quality)
{
    return harc_amd_compress_fastq_files_checked(params, fastq, basedir, preserve_order, preserve_quality, 0);
}
// check (./harc -c -V): the signature (and with -p the order digest) of the reads as ingested, the streams decoded once before they are written, read.check.
// fastq2 (a pair run, harc_amd_compress_fastq_pair_files): the records of fastq followed by those of fastq2 are the job, in that order; read.pair is written
static int compress_fastq_job(const harc_amd_params *params, const char *fastq, const char *fastq2, const char *basedir, int32_t preserve_order, int32_t preserve_quality, int32_t check,
                              uint64_t *records_per_file)
{
    if (!params || !fastq || !basedir) return HARC_AMD_EINVAL;
    for (double &x : g_fastq_timing) x = 0;
    const double t_begin = mono_now();
    // gzip input: only BGZF is read on the GPU; the sniff needs no device, so that the refusal comes first
    double ratio = 1.0;
    const int gz = gzip_kind(fastq, &ratio);
    if (gz < 0) { harc_set_error("%s is gzip but not BGZF: recompress it with bgzip or decompress it first", fastq); return HARC_AMD_EINVAL; }
    const bool bgzf = gz > 0;
    const int gz2 = fastq2 ? gzip_kind(fastq2, nullptr) : 0;       // each file of a pair is sniffed on its own
    if (gz2 < 0) { harc_set_error("%s is gzip but not BGZF: recompress it with bgzip or decompress it first", fastq2); return HARC_AMD_EINVAL; }
    CtxGuard guard; RC_TRY(harc_amd_create(params, &guard.c));
    harc_amd_ctx *const c = guard.c;
    g_fastq_timing[0] = mono_now() - t_begin;
    const double t_ingest = mono_now();
    InFile in; RC_TRY(in.open(fastq));
    FILE *const f = in.f; const uint64_t fsz = in.size;
    const std::string od = std::string(basedir) + "/output/";
    DevBuf d_txt{ c };                                            // -q without -p: the whole text stays in HBM until the orders are known
    IngestState st;
    st.want_third = preserve_quality != 0;                        // every route below ends in ingest_append
    // -q without -p: the text stays in HBM until the orders are known when it fits next to everything else; a larger file is ingested in pieces
    // like any other and streamed again, once per bin of output, when the orders are there (emit_quality_and_ids_streamed)
    bool stream_q = false;
    uint64_t tsz = fsz;                                           // bytes of FASTQ text (BGZF, -q in HBM: known once inflated)
    if (preserve_quality && !preserve_order) {
        size_t fr = 0, tot = 0;
        // BGZF: the text size estimated from the first members, plus what the piece loop holds meanwhile (two compressed pieces, two text buffers)
        const double text_est = bgzf ? ratio * (double)fsz + 2.0 * (1.0 + ratio) * (double)std::min<uint64_t>(fsz, ingest_piece_bytes(true)) : (double)fsz;
        stream_q = (hipMemGetInfo(&fr, &tot) == hipSuccess && text_est > 0.45 * (double)fr);
        if (const char *e = getenv("HARC_AMD_Q_STREAM")) stream_q = atoi(e) != 0;       // tests: either way on a small file
    }
    uint64_t pair_records[2] = { 0, 0 };
    if (fastq2) {                                                 // (always with the order kept: quality values and ids in file order, written while the pieces pass through)
        InFile in2; RC_TRY(in2.open(fastq2));
        QIdFiles out;
        if (preserve_quality) RC_TRY(out.open_pair(od));
        FILE *const ff[2] = { f, in2.f }; const char *const nn[2] = { fastq, fastq2 }; const uint64_t zz[2] = { fsz, in2.size }; const bool bb[2] = { bgzf, gz2 > 0 };
        RC_TRY(ingest_file_pair(c, ff, nn, zz, bb, st, out.fq, out.fi, out.fi2, pair_records));
        if (records_per_file) *records_per_file = pair_records[0];
    } else if (preserve_quality && !preserve_order && !stream_q) {
        if (bgzf) {                                               // the text pieces appended into one buffer
            tsz = 0;
            // sized once from the estimate; grown (with a copy) only where the estimate was short
            RC_TRY(dev_reserve(&d_txt, (size_t)(1.02 * ratio * (double)fsz) + ((size_t)1 << 20)));
            RC_TRY(text_pieces(c, f, fastq, 0, fsz, fsz, true, &g_fastq_timing[2], &g_fastq_timing[8], [&](const char *p, uint64_t n, bool, uint64_t) -> int {
                RC_TRY(dev_reserve(&d_txt, (size_t)(tsz + n), (size_t)tsz));
                HIP_TRY(hipMemcpyAsync(d_txt.p + tsz, p, (size_t)n, hipMemcpyDeviceToDevice, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                tsz += n;
                return HARC_AMD_OK;
            }));
        } else RC_TRY(load_file_range(c, fastq, 0, fsz, &d_txt));
        RC_TRY(ingest_begin(c, st));
        RC_TRY(ingest_append(c, st, d_txt.p, tsz, true, 0, 0));
        RC_TRY(ingest_finish(c, st));
    } else {
        QIdFiles out;
        if (preserve_quality && preserve_order) RC_TRY(out.open(od));          // file order: written while the pieces pass through
        st.want_idlen = stream_q;
        RC_TRY(ingest_file_range(c, f, fastq, 0, fsz, fsz, bgzf, st, out.fq, out.fi));
    }
    g_fastq_timing[1] = mono_now() - t_ingest;
    printf("Read length: %d\nTotal number of reads: %llu\nTotal number of reads without N: %llu\nPreprocessing Done!\n", params->readlen,
           (unsigned long long)st.nfull, (unsigned long long)c->N);                                       // preprocess.cpp:133-136
    LapTimer tm{ "[compress_fastq]" };
    RC_TRY(spit_stream(c, HARC_AMD_IN_ORDER_N, 0, od + "read_order_N.bin"));
    { const uint32_t n32 = c->N; RC_TRY(spit_file(od + "numreads.bin", &n32, 4)); }
    uint64_t sig_in[3] = { 0, 0, 0 }, t_order[3] = { 0, 0, 0 };
    if (check) {                                                  // of the input as ingested, before a stage has touched it
        RC_TRY(harc_amd_input_signature(c, sig_in));
        if (preserve_order) RC_TRY(harc_amd_input_order_digest(c, t_order));
        tm.lap("input signature");
    }
    double t_ph = mono_now();
    RC_TRY(harc_amd_reorder(c));
    tm.lap("reorder");
    g_fastq_timing[4] = mono_now() - t_ph; t_ph = mono_now();
    RC_TRY(harc_amd_encode(c));
    tm.lap("encode");
    g_fastq_timing[5] = mono_now() - t_ph; t_ph = mono_now();
    harc_amd_counters C; harc_amd_get_counters(c, &C);
    printf("Reordering done, %llu were unmatched\n", (unsigned long long)C.unmatched);
    printf("Encoding done:\n%llu singleton reads were aligned\n%llu reads with N were aligned\n", (unsigned long long)C.aligned_singletons, (unsigned long long)C.aligned_N);
    if (check) {                                                  // the streams are decoded once before a byte of them is written
        uint64_t sig_out[3] = { 0, 0, 0 };
        RC_TRY(harc_amd_decode_signature(c, sig_out));
        tm.lap("streams decoded");
        if (memcmp(sig_in, sig_out, sizeof sig_in)) {
            harc_set_error("the streams do not decode to the reads that came in: the input's signature is (%016llx, %016llx, %016llx), the decoded streams' is (%016llx, %016llx, %016llx); nothing was written",
                           (unsigned long long)sig_in[0], (unsigned long long)sig_in[1], (unsigned long long)sig_in[2], (unsigned long long)sig_out[0], (unsigned long long)sig_out[1], (unsigned long long)sig_out[2]);
            return HARC_AMD_EINTERNAL;
        }
        char rec[256]; int k = snprintf(rec, sizeof rec, "%s\n", CK_MAGIC);
        k += ck_format_reads(rec + k, sizeof rec - (size_t)k, sig_in);
        if (preserve_order) k += ck_format_order(rec + k, sizeof rec - (size_t)k, t_order);
        RC_TRY(spit_file(od + "read.check", rec, (size_t)k));
    }
    if (fastq2) {                                                 // the record of a pair run; ./harc appends the line "ids <rule>" with -q
        char rec[64]; const int k = snprintf(rec, sizeof rec, "HARCP1\nrecords %llu\n", (unsigned long long)pair_records[0]);
        RC_TRY(spit_file(od + "read.pair", rec, (size_t)k));
    }
    if (preserve_quality) {                                       // the record of the third lines: only when they are not bare, so that such an archive is what it always was
        const int32_t third = th_rule_of(st.third_and, st.third_n);
        if (third != TH_BARE) {
            char rec[64]; const int k = snprintf(rec, sizeof rec, "%s\nthird %s\n", TH_MAGIC, th_rule_name(third));
            RC_TRY(spit_file(od + "read.third", rec, (size_t)k));
        }
        if (third == TH_DROPPED) printf("[third] the input's third lines carry text that is not their ids; it is not kept (-d -q writes a bare + in its place)\n");
    }
    RC_TRY(write_shard_family(c, od, 0));
    tm.lap("stream files");
    RC_TRY(write_whole_job_files(c, od));
    g_fastq_timing[6] = mono_now() - t_ph; g_fastq_timing[7] = mono_now() - t_begin;
    if (preserve_quality && !preserve_order) {
        printf("Reordering quality values and ids\n");                                                      // harc:122
        tm.lap("whole-job files");
        if (stream_q) RC_TRY(emit_quality_and_ids_streamed(c, f, fastq, fsz, bgzf, st, od));
        else RC_TRY(emit_quality_and_ids(c, d_txt.p, tsz, st, od));
        tm.lap("quality values and ids");
    }
    return HARC_AMD_OK;
}
extern "C" int harc_amd_compress_fastq_files_checked(const harc_amd_params *params, const char *fastq, const char *basedir, int32_t preserve_order, int32_t preserve_quality, int32_t check)
{
    return compress_fastq_job(params, fastq, nullptr, basedir, preserve_order, preserve_quality, check, nullptr);
}
extern "C" int harc_amd_compress_fastq_pair_files(const harc_amd_params *params, const char *fastq1, const char *fastq2, const char *basedir, int32_t preserve_quality, int32_t check,
                                                  uint64_t *records_per_file)
{
    if (!fastq2) { harc_set_error("compress_fastq_pair_files: bad arguments"); return HARC_AMD_EINVAL; }
    return compress_fastq_job(params, fastq1, fastq2, basedir, 1, preserve_quality, check, records_per_file);
}
extern "C" int harc_amd_compress_fastq_files(const harc_amd_params *params, const char *fastq, const char *basedir)
{
    return harc_amd_compress_fastq_files_ex(params, fastq, basedir, 0, 0);
}

// ------------------------------------------------------------------------------------------------ one rank of a multi-GPU run
static int rendezvous(harc_amd_ctx *c, const char *spec, int world, int rank)
{
    if (!spec) { harc_set_error("comm_spec missing"); return HARC_AMD_EINVAL; }
    if (!strncmp(spec, "mailbox:", 8)) return harc_amd_comm_init_mailbox(c, spec + 8, world, rank);
    if (strncmp(spec, "rccl:", 5)) { harc_set_error("comm_spec must be rccl:<file> or mailbox:<dir>"); return HARC_AMD_EINVAL; }
    const std::string path = spec + 5;
    uint8_t id[HARC_AMD_COMM_ID_BYTES];
    if (rank == 0) {
        RC_TRY(harc_amd_comm_get_id(id, sizeof id));
        RC_TRY(spit_file(path + ".tmp", id, sizeof id));
        if (rename((path + ".tmp").c_str(), path.c_str()) != 0) { harc_set_error("cannot publish %s", path.c_str()); return HARC_AMD_EIO; }
    } else {
        FILE *f = nullptr;
        for (int tries = 0; !(f = fopen(path.c_str(), "rb")); tries++) {
            if (tries > 150000) { harc_set_error("rank %d: no communicator id at %s after 300 s", rank, path.c_str()); return HARC_AMD_EIO; }
            usleep(2000);
        }
        const bool ok = fread(id, 1, sizeof id, f) == sizeof id;
        fclose(f);
        if (!ok) { harc_set_error("short communicator id in %s", path.c_str()); return HARC_AMD_EIO; }
    }
    return harc_amd_comm_init(c, id, sizeof id, world, rank);
}

static int compress_fastq_rank(const harc_amd_params *params, const char *fastq, const char *basedir, int32_t preserve_order,
                               int32_t preserve_quality, int32_t world, int32_t rank, const char *comm_spec, bool replicate);
extern "C" int harc_amd_compress_fastq_shard_files(const harc_amd_params *params, const char *fastq, const char *basedir, int32_t preserve_order,
                                                   int32_t preserve_quality, int32_t world, int32_t rank, const char *comm_spec)
{
    return compress_fastq_rank(params, fastq, basedir, preserve_order, preserve_quality, world, rank, comm_spec, false);
}
// design (R): every rank ingests its slice, the reads are all-gathered, the chains partitioned; every rank ends with the streams of the whole
// job -- ONE GPU's streams, byte for byte -- and rank 0 writes them (as shard family 0 .. num_thr - 1, like a single-GPU run); what depends on
// the slice (read_order_N.bin, quality values and ids in file order) is left as rank parts.  harc_amd_merge_shard_files finishes the archive.
extern "C" int harc_amd_compress_fastq_replicated_files(const harc_amd_params *params, const char *fastq, const char *basedir, int32_t preserve_order,
                                                        int32_t preserve_quality, int32_t world, int32_t rank, const char *comm_spec)
{
    return compress_fastq_rank(params, fastq, basedir, preserve_order, preserve_quality, world, rank, comm_spec, true);
}
static int compress_fastq_rank(const harc_amd_params *params, const char *fastq, const char *basedir, int32_t preserve_order,
                               int32_t preserve_quality, int32_t world, int32_t rank, const char *comm_spec, bool replicate)
{
    if (!params || !fastq || !basedir || world < 1 || rank < 0 || rank >= world) { harc_set_error("compress_fastq_shard: bad arguments"); return HARC_AMD_EINVAL; }
    if (preserve_quality && !preserve_order) { harc_set_error("multi-GPU -q needs -p (quality values and ids stay in file order)"); return HARC_AMD_EINVAL; }
    if (gzip_kind(fastq, nullptr) != 0) { harc_set_error("multi-GPU runs read a plain FASTQ: %s is gzip / BGZF, expand it first", fastq); return HARC_AMD_EINVAL; }
    CtxGuard guard; RC_TRY(harc_amd_create(params, &guard.c));
    harc_amd_ctx *const c = guard.c;
    InFile in; RC_TRY(in.open(fastq));
    FILE *const f = in.f; const uint64_t fsz = in.size;
    uint64_t lo = 0, hi = fsz;
    RC_TRY(record_start_at_or_after(f, fsz / (uint64_t)world * (uint64_t)rank, fsz, &lo));
    if (rank + 1 < world) RC_TRY(record_start_at_or_after(f, fsz / (uint64_t)world * (uint64_t)(rank + 1), fsz, &hi));
    const std::string od = std::string(basedir) + "/output/", sd = od + ".shard/", r = "." + std::to_string(rank);
    (void)mkdir(sd.c_str(), 0777);                                // every rank tries; the first one wins
    IngestState st;
    {
        QIdFiles out;
        if (preserve_quality) RC_TRY(out.open_parts(sd, r));      // file order (preprocess.cpp:64-69): the slices are concatenated by the merge
        RC_TRY(ingest_file_range(c, f, fastq, lo, hi, fsz, false, st, out.fq, out.fi));
    }
    const uint64_t nrec_full = st.nfull;
    const uint64_t n_clean_own = c->N_own;
    std::vector<uint32_t> orderN = st.orderN;                     // read_order_N.bin of this slice, local record numbers
    RC_TRY(rendezvous(c, comm_spec, world, rank));
    uint64_t info[8];
    if (replicate) RC_TRY(harc_amd_replicate_exchange(c, info)); else RC_TRY(harc_amd_shard_exchange(c, info));
    for (auto &x : orderN) x += (uint32_t)info[5];                // records of the lower ranks come first in the file
    RC_TRY(spit_file(sd + "order_N" + r, orderN.data(), orderN.size() * 4));
    RC_TRY(harc_amd_reorder(c));
    RC_TRY(harc_amd_encode(c));
    harc_amd_counters C; harc_amd_get_counters(c, &C);
    if (replicate && rank != 0 && !c->s2_part) {                  // (HARC_AMD_S2_PART=0) the same streams as rank 0 holds: nothing to write but empty parts
        static const char *stems[] = { "order_a", "order_u", "orderN_a", "orderN_u", "singleton", "singleton_tail", "input_N" };
        for (const char *st0 : stems) RC_TRY(spit_file(sd + st0 + r, "", 0));
        char line[256];
        const int n = snprintf(line, sizeof line, "%d %llu %llu %llu 0 0 0 %llu %llu\n", params->readlen, (unsigned long long)nrec_full,
                               (unsigned long long)n_clean_own, (unsigned long long)c->NN_own, (unsigned long long)c->N, (unsigned long long)c->NN);
        RC_TRY(spit_file(sd + "stats" + r, line, (size_t)n));
        RC_TRY(harc_amd_comm_barrier(c));
        return HARC_AMD_OK;
    }
    // design (R) with stage II partitioned: every rank writes the stream files of ITS encoder shards under their single-GPU names, and its parts of
    // the whole-job files (aligned part: its shards; unaligned part: its share of the candidates) -- the merge below is the bucket mode's
    if (replicate && c->s2_part) {
        RC_TRY(write_shard_family(c, od, 0, c->s2_e0, c->s2_e1));
        if (rank != 0) C.unmatched = 0;                           // stage I is the whole job's on every rank: counted once
    } else
    RC_TRY(write_shard_family(c, od, replicate ? 0 : rank * params->num_thr));
    {   // whole-job files: this rank's part, aligned and unaligned halves apart (the merge interleaves them as encoder.cpp:457-503 does)
        const void *po, *pn, *ps, *pt, *pi; size_t no, nn, ns, nt, ni;
        RC_TRY(harc_amd_get_stream(c, HARC_AMD_S2_ORDER, 0, &po, &no)); RC_TRY(harc_amd_get_stream(c, HARC_AMD_S2_ORDER_N_PE, 0, &pn, &nn));
        RC_TRY(harc_amd_get_stream(c, HARC_AMD_S2_SINGLETON, 0, &ps, &ns)); RC_TRY(harc_amd_get_stream(c, HARC_AMD_S2_SINGLETON_TAIL, 0, &pt, &nt));
        RC_TRY(harc_amd_get_stream(c, HARC_AMD_S2_INPUT_N, 0, &pi, &ni));
        const int L = params->readlen;
        const size_t US = (4 * ns + nt) / (size_t)L, UN = ni / (size_t)(L + 1);
        if (no < US * 4 || nn < UN * 4) { harc_set_error("shard %d: order streams shorter than the unaligned reads", rank); return HARC_AMD_ESTATE; }
        RC_TRY(spit_file(sd + "order_a" + r, po, no - US * 4)); RC_TRY(spit_file(sd + "order_u" + r, (const char *)po + (no - US * 4), US * 4));
        RC_TRY(spit_file(sd + "orderN_a" + r, pn, nn - UN * 4)); RC_TRY(spit_file(sd + "orderN_u" + r, (const char *)pn + (nn - UN * 4), UN * 4));
        RC_TRY(spit_file(sd + "singleton" + r, ps, ns)); RC_TRY(spit_file(sd + "singleton_tail" + r, pt, nt));
        RC_TRY(spit_file(sd + "input_N" + r, pi, ni));
    }
    {
        char line[512];
        const int n = snprintf(line, sizeof line, "%d %llu %llu %llu %llu %llu %llu %llu %llu\n", params->readlen, (unsigned long long)nrec_full,
                               (unsigned long long)n_clean_own, (unsigned long long)c->NN_own, (unsigned long long)C.unmatched,
                               (unsigned long long)C.aligned_singletons, (unsigned long long)C.aligned_N, (unsigned long long)c->N, (unsigned long long)c->NN);
        RC_TRY(spit_file(sd + "stats" + r, line, (size_t)n));       // written last: its presence says that the rank is done
    }
    RC_TRY(harc_amd_comm_barrier(c));                             // nobody leaves (and tears the communicator down) while a peer is still exchanging
    return HARC_AMD_OK;
}
