// check.hip -- the digests behind ./harc -c -V, -d and -v (README: "-V and what it promises").  The arithmetic is check_block.h's; this file gives it its lanes,
// reduces what the lanes summed, and holds the calls of the C-ABI.
//   k_text_digest    a text as one streaming pass: aligned 16-byte loads over the 16-byte hull of the text (a lane masks the bytes of the first and the last
//                    chunk that are not the text's), sixteen terms a lane and iteration in registers, a reduction across the wave, one 64-bit atomic add per wave
//                    and word.  Integer sums: the result does not depend on the grid, the pieces or the order of the atomics.
//   k_order_digest   T of the text "read_0\nread_1\n..." in input record order, from what the ingest left in the context: the packed clean reads, the packed
//                    reads with N and the record numbers of the latter.  A lane per record; the record is a read with N when a binary search finds its number.
#include "devutil.h"
#include "check_block.h"
#include "fileio.h"

#define CK_T 256

// d and nl of every lane of the wave -> acc[0] (newlines) and acc[1] (D)
__device__ __forceinline__ void ck_wave_flush(uint64_t d, uint64_t nl, unsigned long long *acc)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { d += shfl_u64_any(d, o); nl += shfl_u64_any(nl, o); }
    if ((threadIdx.x & 63u) == 0) {
        if (nl) atomicAdd(&acc[0], (unsigned long long)nl);
        if (d) atomicAdd(&acc[1], (unsigned long long)d);
    }
}

// the n > 0 bytes at p, byte i at offset first + i of the whole text
__global__ __launch_bounds__(CK_T) void k_text_digest(const uint8_t *p, uint64_t n, uint64_t first, unsigned long long *acc)
{
    const uint64_t mis = (uint64_t)((uintptr_t)p & 15u), hull = mis + n, nchunks = (hull + 15) >> 4;
    const uint4 *base = (const uint4 *)(p - mis);
    uint64_t d = 0; uint32_t nl = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * CK_T + threadIdx.x; k < nchunks; k += (uint64_t)gridDim.x * CK_T) {
        const uint4 v = base[k];
        const uint64_t a = k << 4;                                // the chunk's first byte, counted from the hull's
        uint32_t keep = 0xFFFFu;
        if (a < mis) keep &= 0xFFFFu << (uint32_t)(mis - a);      // (chunk 0 alone)
        if (a + 16 > hull) keep &= 0xFFFFu >> (uint32_t)(a + 16 - hull);
        const uint64_t pos = first + a - mis;                     // of the chunk's byte 0; modulo 2^64 where that byte lies in front of the text (it is masked)
        ck_word((uint64_t)v.x | ((uint64_t)v.y << 32), keep & 0xFFu, pos, &d, &nl);
        ck_word((uint64_t)v.z | ((uint64_t)v.w << 32), keep >> 8, pos + 8, &d, &nl);
    }
    ck_wave_flush(d, nl, acc);
}

// record r of nrec = n2 + n3 records: the read with N number m when orderN[m] == r (orderN ascending), else the clean read number r - (reads with N in front of it)
__global__ __launch_bounds__(CK_T) void k_order_digest(const uint64_t *reads2, uint32_t n2, int W, const uint64_t *reads3, uint32_t n3, int W3, const uint32_t *orderN,
                                                       uint64_t nrec, int L, unsigned long long *acc, unsigned int *err)
{
    const uint64_t r = harc_gid();
    uint64_t d = 0;
    if (r < nrec) {
        uint32_t lo = 0, hi = n3;                                 // lower bound of r in orderN
        while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if ((uint64_t)orderN[mid] < r) lo = mid + 1; else hi = mid; }
        const bool isN = lo < n3 && (uint64_t)orderN[lo] == r;
        const uint64_t pos = r * (uint64_t)(L + 1);
        if (isN) {
            const uint64_t *w = reads3 + (size_t)lo * W3;
            for (int j = 0; j < L; j++) {
                const int off = 3 * j, wi = off >> 6, sh = off & 63;
                uint64_t v = w[wi] >> sh;
                if (sh > 61 && wi + 1 < W3) v |= w[wi + 1] << (64 - sh);
                const int c3 = (int)(v & 7);
                d += ck_term(pos + j, c3 == 0 ? 'A' : c3 == 4 ? 'C' : c3 == 2 ? 'G' : c3 == 6 ? 'T' : 'N');
            }
        } else if (r - lo < (uint64_t)n2) {
            const uint64_t *w = reads2 + (size_t)(r - lo) * W;
            for (int j = 0; j < L; j++) { const int pc = (int)((w[j >> 5] >> (2 * (j & 31))) & 3); d += ck_term(pos + j, pc == 0 ? 'A' : pc == 1 ? 'G' : pc == 2 ? 'C' : 'T'); }
        } else atomicAdd(err, 1u);                                // the record numbers of the reads with N do not fit the counts
        d += ck_term(pos + L, '\n');
    }
    ck_wave_flush(d, 0, acc);
}

// the piece on the context's stream, its newlines and D terms added to the two device words at `slots`; nothing is waited for
static int ck_launch(harc_amd_ctx *c, const void *d_text, uint64_t n, uint64_t first, unsigned long long *slots)
{
    if (!n) return HARC_AMD_OK;
    const uint64_t nchunks = (n + 15 + 15) >> 4;                  // at most: the hull of a text that starts at byte 15 of a chunk
    uint64_t blocks = (nchunks + CK_T * 4 - 1) / (CK_T * 4);      // four chunks a lane, up to eight workgroups a CU
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_text_digest, dim3((unsigned)blocks), dim3(CK_T), 0, c->stream, (const uint8_t *)d_text, n, first, slots);
    HIP_TRY(hipGetLastError());
    return HARC_AMD_OK;
}
// two cleared device words out of the pool (the caller's PoolScope)
static int ck_slots(harc_amd_ctx *c, unsigned long long **slots)
{
    RC_TRY(dalloc(c, slots, 2));
    HIP_TRY(hipMemsetAsync(*slots, 0, 16, c->stream));
    return HARC_AMD_OK;
}
static int ck_fetch(harc_amd_ctx *c, const unsigned long long *slots, uint64_t bytes, uint64_t acc[3])
{
    unsigned long long h[2] = { 0, 0 };
    HIP_TRY(hipMemcpyAsync(h, slots, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    acc[0] += bytes; acc[1] += h[0]; acc[2] += h[1];
    return HARC_AMD_OK;
}

extern "C" int harc_amd_text_digest_device(harc_amd_ctx *c, const void *d_text, uint64_t nbytes, uint64_t first_offset, uint64_t *acc)
{
    if (!c || !acc || (nbytes && !d_text)) { harc_set_error("text_digest_device: bad arguments"); return HARC_AMD_EINVAL; }
    if (!nbytes) return HARC_AMD_OK;
    HIP_TRY(hipSetDevice(c->P.device));
    PoolScope scope(c);
    unsigned long long *slots = nullptr;
    RC_TRY(ck_slots(c, &slots));
    const bool trace = getenv("HARC_AMD_TRACE") != nullptr;
    double seconds = 0;
    KernelTimer timer(trace ? &seconds : nullptr);
    RC_TRY(timer.begin(c->stream));
    RC_TRY(ck_launch(c, d_text, nbytes, first_offset, slots));
    RC_TRY(timer.end_mark(c->stream));
    RC_TRY(ck_fetch(c, slots, nbytes, acc));
    RC_TRY(timer.end_wait());
    if (trace) fprintf(stderr, "[check] device call: %llu bytes of text, kernel %.3f ms (%.1f GB/s of text)\n", (unsigned long long)nbytes, 1e3 * seconds, seconds > 0 ? 1e-9 * (double)nbytes / seconds : 0.0);
    return HARC_AMD_OK;
}

extern "C" int harc_amd_text_digest_host(const void *text, uint64_t nbytes, uint64_t first_offset, uint64_t *acc)
{
    if (!acc || (nbytes && !text)) { harc_set_error("text_digest_host: bad arguments"); return HARC_AMD_EINVAL; }
    ck_digest_host((const uint8_t *)text, nbytes, first_offset, acc);
    return HARC_AMD_OK;
}

extern "C" int harc_amd_input_order_digest(harc_amd_ctx *c, uint64_t *out)
{
    if (!c || !out) { harc_set_error("input_order_digest: bad arguments"); return HARC_AMD_EINVAL; }
    HIP_TRY(hipSetDevice(c->P.device));
    const int L = c->P.readlen;
    const uint64_t nrec = (uint64_t)c->N + c->NN;
    out[0] = nrec * (uint64_t)(L + 1); out[1] = nrec; out[2] = 0;
    if (!nrec) return HARC_AMD_OK;
    if ((c->N && !c->d_reads) || (c->NN && !c->d_nreads3)) { harc_set_error("input_order_digest: the context holds no reads"); return HARC_AMD_ESTATE; }
    auto it = c->out.find(std::make_pair((int)HARC_AMD_IN_ORDER_N, 0));
    const std::vector<uint8_t> *on = it == c->out.end() ? nullptr : &it->second.own;
    if ((on ? on->size() : 0) != (size_t)c->NN * 4) { harc_set_error("input_order_digest: the context holds %u reads with N and %zu of their record numbers (set by harc_amd_set_fastq_device)", c->NN, on ? on->size() / 4 : (size_t)0); return HARC_AMD_ESTATE; }
    PoolScope scope(c);
    unsigned long long *slots = nullptr; uint32_t *d_on = nullptr; unsigned int *d_err = nullptr;
    RC_TRY(ck_slots(c, &slots));
    RC_TRY(dalloc(c, &d_on, (size_t)c->NN + 1)); RC_TRY(dalloc(c, &d_err, 4));
    HIP_TRY(hipMemsetAsync(d_err, 0, 16, c->stream));
    if (c->NN) HIP_TRY(hipMemcpyAsync(d_on, on->data(), (size_t)c->NN * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_order_digest, harc_grid256(nrec), dim3(CK_T), 0, c->stream, (const uint64_t *)c->d_reads, c->N, c->W, (const uint64_t *)c->d_nreads3, c->NN, c->W3, (const uint32_t *)d_on, nrec, L,
                       slots, d_err);
    HIP_TRY(hipGetLastError());
    unsigned int err = 0; uint64_t acc[3] = { 0, 0, 0 };
    HIP_TRY(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, c->stream));
    RC_TRY(ck_fetch(c, slots, 0, acc));
    if (err) { harc_set_error("input_order_digest: %u records are neither a clean read nor a read with N: the record numbers of the reads with N do not fit the counts", err); return HARC_AMD_EINTERNAL; }
    out[2] = acc[2];
    return HARC_AMD_OK;
}

// ------------------------------------------------------------------------------------------------ the files
extern "C" int harc_amd_text_digest_files(const harc_amd_params *params, const char *path, uint64_t *out)
{
    if (!params || !path || !out) { harc_set_error("text_digest_files: bad arguments"); return HARC_AMD_EINVAL; }
    uint64_t fsz = 0;
    if (!file_size(path, &fsz)) { harc_set_error("cannot open %s", path); return HARC_AMD_EIO; }
    out[0] = out[1] = out[2] = 0;
    if (!fsz) return HARC_AMD_OK;
    CtxGuard guard;
    RC_TRY(side_context(params, 100, &guard.c));
    harc_amd_ctx *c = guard.c;
    RingGeom g;
    RC_TRY(ring_split(c, 1, 16, "check", &g, ring_slice_for(fsz, 16)));
    const uint64_t piece = (uint64_t)64 << 20;
    const Pieces pieces = byte_pieces(0, fsz, piece);
    DevBuf txt{ c };
    RC_TRY(dev_reserve(&txt, (size_t)(fsz < piece ? fsz : piece)));
    PoolScope scope(c);
    unsigned long long *slots = nullptr;
    RC_TRY(ck_slots(c, &slots));
    const bool tlog = getenv("HARC_AMD_TRACE") != nullptr;
    double t_read = 0, t_kernel = 0; const double t0 = mono_now();
    {
        FileFeeder feed(c, path);
        RC_TRY(feed.start(pieces, g));
        KernelTimer timer(tlog ? &t_kernel : nullptr);
        for (size_t p = 0; p < pieces.size(); p++) {              // the kernel of piece p and the uploads of piece p + 1 follow each other on the stream: one buffer
            { const double tr = mono_now(); RC_TRY(feed.upload_piece(p, txt.p, nullptr)); t_read += mono_now() - tr; }
            RC_TRY(timer.begin(c->stream));
            RC_TRY(ck_launch(c, txt.p, pieces[p].second - pieces[p].first, pieces[p].first, slots));
            RC_TRY(timer.end(c->stream));
        }
        RC_TRY(ck_fetch(c, slots, fsz, out));
    }
    if (tlog) fprintf(stderr, "[check] %llu bytes of text in %zu pieces, %.3f s: %.3f s in the kernels, %.3f s waiting for the readers\n", (unsigned long long)fsz, pieces.size(), mono_now() - t0, t_kernel, t_read);
    return HARC_AMD_OK;
}

// dna_path (what the decoders write: fixed-length reads, one per line) read once: sig = the multiset signature of its reads (verify.hip), t = T of its text
extern "C" int harc_amd_reads_check_files(const harc_amd_params *params, const char *dna_path, uint64_t *sig, uint64_t *t)
{
    if (!params || !dna_path || !sig || !t) { harc_set_error("reads_check_files: bad arguments"); return HARC_AMD_EINVAL; }
    uint64_t fsz = 0;
    if (!file_size(dna_path, &fsz)) { harc_set_error("cannot open %s", dna_path); return HARC_AMD_EIO; }
    sig[0] = sig[1] = sig[2] = 0; t[0] = t[1] = t[2] = 0;
    if (!fsz) return HARC_AMD_OK;
    uint32_t L = 1;
    RC_TRY(first_line_length(dna_path, "reads_check_files", &L));
    const uint64_t LL = L + 1ull;
    if (fsz % LL) { harc_set_error("reads_check_files: %s holds %llu bytes, no multiple of the %llu bytes of a read of %u bases and its newline", dna_path, (unsigned long long)fsz, (unsigned long long)LL, L); return HARC_AMD_EINVAL; }
    const uint64_t n = fsz / LL;
    CtxGuard guard;
    RC_TRY(side_context(params, (int)L, &guard.c));
    harc_amd_ctx *c = guard.c;
    RingGeom g;
    RC_TRY(ring_split(c, 1, 16, "check", &g, ring_slice_for(fsz, 16)));
    const uint64_t dflt = ((uint64_t)64 << 20) / LL, piece_lines = dflt ? dflt : 1;
    const Pieces pieces = line_pieces(n, LL, piece_lines);
    DevBuf txt{ c };
    RC_TRY(dev_reserve(&txt, (size_t)(pieces[0].second - pieces[0].first)));
    PoolScope scope(c);
    unsigned long long *slots = nullptr;
    RC_TRY(ck_slots(c, &slots));
    FileFeeder feed(c, dna_path);
    RC_TRY(feed.start(pieces, g));
    for (size_t p = 0; p < pieces.size(); p++) {
        const uint64_t bytes = pieces[p].second - pieces[p].first;
        RC_TRY(feed.upload_piece(p, txt.p, nullptr));
        RC_TRY(ck_launch(c, txt.p, bytes, pieces[p].first, slots));
        uint64_t s[3] = { 0, 0, 0 };
        RC_TRY(harc_amd_reads_signature_device(c, txt.p, (uint32_t)(bytes / LL), (uint32_t)LL, s));       // (waits for the stream)
        sig[0] += s[0]; sig[1] += s[1]; sig[2] ^= s[2];
    }
    return ck_fetch(c, slots, fsz, t);
}
