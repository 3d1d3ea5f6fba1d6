// verify.hip -- decode side on the GPU, used as the size-independent round-trip check.
//
// decoder.cpp:90-169 restated data-parallel: the start column of read i in its shard's consensus stream is (sum of the pos bytes
// up to i) - readlen, its noise entries sit between the (i-1)-th and i-th '\n' of read_noise, the mismatch positions are the
// running sum of its read_noisepos bytes (decoder.cpp:100-108), the read is reverse-complemented when its read_rev bit is set
// (:109-129).  Instead of writing 100 B per read back to the host, every decoded read is hashed and the hashes are summed and
// xored: an order-independent signature of the decoded multiset that is compared with the same signature of the input reads.
#include "devutil.h"
#include "fileio.h"

__device__ __forceinline__ uint64_t read_hash_step(uint64_t h, int code) { return (h ^ (uint64_t)code) * 1099511628211ULL; }   // FNV-1a over codes A0 C1 G2 T3 N4
#define READ_HASH_INIT 1469598103934665603ULL

__device__ __forceinline__ void sig_accumulate(uint64_t h, bool valid, unsigned long long *sig)
{
    // sig[0] count, sig[1] sum, sig[2] xor ; wave-level reduction first
    unsigned long long s = valid ? h : 0, x = valid ? h : 0, n = valid ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += shfl_u64_any(s, o); x ^= shfl_u64_any(x, o); n += shfl_u64_any(n, o);
    }
    if ((threadIdx.x & 63) == 0 && n) { atomicAdd(&sig[0], n); atomicAdd(&sig[1], s); atomicXor(&sig[2], x); }
}

__global__ void k_sig_ascii(const char *ascii, uint32_t n, uint32_t stride, int L, unsigned long long *sig)
{
    const uint32_t i = harc_gid32();
    uint64_t h = READ_HASH_INIT;
    if (i < n) {
        const char *s = ascii + (size_t)i * stride;
        for (int j = 0; j < L; j++) { const char ch = s[j]; h = read_hash_step(h, ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4); }
        h = mix64(h);
    }
    sig_accumulate(h, i < n, sig);
}
// 2-bit packed stream (A0 C1 G2 T3, 4 per byte, encoder.cpp:540-541) + ASCII tail -> one code per byte
__global__ void k_unpack_seq(const uint8_t *packed, uint64_t nb, const uint8_t *tail, uint64_t ntail, uint8_t *out)
{
    const uint64_t i = harc_gid();
    if (i < 4 * nb) out[i] = (packed[i >> 2] >> (2 * (i & 3))) & 3;
    else if (i < 4 * nb + ntail) { const uint8_t ch = tail[i - 4 * nb]; out[i] = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : 3; }
}
__global__ void k_pos_to_u64(const uint8_t *pos, uint32_t n, uint64_t *out)
{
    const uint32_t i = harc_gid32();
    if (i < n) out[i] = pos[i];
}
__global__ void k_nl_flags(const uint8_t *noise, uint64_t n, uint32_t *flag)
{
    const uint64_t i = harc_gid();
    if (i < n) flag[i] = noise[i] == '\n' ? 1u : 0u;
}
__global__ void k_nl_positions(const uint8_t *noise, const uint32_t *rank, uint64_t n, uint64_t *nlpos)
{
    const uint64_t i = harc_gid();
    if (i < n && noise[i] == '\n') nlpos[rank[i]] = i;
}
// Read i of a shard into buf[0 .. L) as codes A0 C1 G2 T3 N4, in the direction of the consensus; *rev: the read is its reverse complement (decoder.cpp:109-129).
// false: the read's span does not lie inside the consensus stream, nothing was decoded.  That, a mismatch position outside the read and a noise code outside
// '0'..'3' are each counted into *err: the host refuses the archive.  nlpos[i] and the noisepos bytes of the read exist because the host has checked the line
// count of `noise` and the length of `noisepos` before the launch (shard_prepare).
__device__ __forceinline__ bool decode_read(const uint8_t *seqb, uint64_t seqlen, const uint64_t *possum, const uint8_t *noise, const uint8_t *noisepos,
                                            const uint64_t *nlpos, const uint8_t *revb, uint64_t nrevb, const uint8_t *revtail, uint32_t i, int L,
                                            uint8_t *buf, bool *rev, bool *hasN, unsigned int *err)
{
    const uint64_t start = possum[i] - (uint64_t)L;                           // decoder.cpp:93-98
    if (possum[i] < (uint64_t)L || start + L > seqlen) { atomicAdd(err, 1u); return false; }
    for (int j = 0; j < L; j++) buf[j] = seqb[start + j];
    const uint64_t n0 = i ? nlpos[i - 1] + 1 : 0, n1 = nlpos[i];
    uint64_t np = n0 - i;                                                     // noisepos bytes consumed by earlier reads
    int p = 0; bool wroteN = false;
    for (uint64_t k = n0; k < n1; k++) {                                      // decoder.cpp:100-108
        if (p < L) p += noisepos[np];                                         // (a position past the read stays there: p never exceeds L + 254, buf is never indexed with it)
        np++;
        const int code = noise[k] - '0';
        if (p >= L || (unsigned)code > 3u) { atomicAdd(err, 1u); continue; }
        const int ref = seqb[start + p] & 3;                                  // the row of the CONSENSUS base (dec_noise[ref[noisepos]], :106), also where a position is named twice
        // dec_noise (decoder.cpp setglobalarrays): A:{C,G,T,N} C:{A,G,T,N} G:{T,A,C,N} T:{G,C,A,N}
        const unsigned tab = ref == 0 ? 0x4321u : ref == 1 ? 0x4320u : ref == 2 ? 0x4103u : 0x4012u;
        buf[p] = (uint8_t)((tab >> (4 * code)) & 0xF); wroteN |= code == 3;
    }
    *rev = i < 8 * nrevb ? ((revb[i >> 3] >> (i & 7)) & 1) : (revtail[i - 8 * nrevb] == 'r');
    bool anyN = false;                                                        // strchr(currentread, 'N') on the finished read (:110): a later entry may have taken an N away again
    if (wroteN) for (int j = 0; j < L; j++) anyN |= buf[j] == 4;
    *hasN = anyN;
    return true;
}
// one thread per read of a shard: decode, hash; a read that could not be decoded is left out of the signature
__global__ void k_decode_sig(const uint8_t *seqb, uint64_t seqlen, const uint64_t *possum, const uint8_t *noise, const uint8_t *noisepos,
                             const uint64_t *nlpos, const uint8_t *revb, uint64_t nrevb, const uint8_t *revtail, uint32_t n, int L,
                             unsigned long long *sig, unsigned int *err)
{
    const uint32_t i = harc_gid32();
    uint64_t h = READ_HASH_INIT;
    uint8_t buf[256]; bool rev = false, hasN;
    const bool ok = i < n && decode_read(seqb, seqlen, possum, noise, noisepos, nlpos, revb, nrevb, revtail, i, L, buf, &rev, &hasN, err);
    if (ok) {
        if (!rev) for (int j = 0; j < L; j++) h = read_hash_step(h, buf[j]);
        else for (int j = L - 1; j >= 0; j--) h = read_hash_step(h, buf[j] == 4 ? 4 : 3 - buf[j]);   // decoder.cpp:109-129
        h = mix64(h);
    }
    sig_accumulate(h, ok, sig);
}
// unaligned singletons: 2-bit packed, L bases each, back to back (encoder.cpp:484-491)
__global__ void k_sig_codes(const uint8_t *codes, uint32_t n, int L, unsigned long long *sig)
{
    const uint32_t i = harc_gid32();
    uint64_t h = READ_HASH_INIT;
    if (i < n) { for (int j = 0; j < L; j++) h = read_hash_step(h, codes[(size_t)i * L + j]); h = mix64(h); }
    sig_accumulate(h, i < n, sig);
}
// the two file decoders: the same decode as k_decode_sig, but the read is written as a text line into tmp[i] and flagged when it contains N
// (decoder.cpp:110-129 routes those to a separate file that is appended after the singletons, :141-169).
__global__ void k_decode_text(const uint8_t *seqb, uint64_t seqlen, const uint64_t *possum, const uint8_t *noise, const uint8_t *noisepos,
                              const uint64_t *nlpos, const uint8_t *revb, uint64_t nrevb, const uint8_t *revtail, uint32_t n, int L,
                              char *tmp, uint32_t *isN, unsigned int *err)
{
    const uint32_t i = harc_gid32();
    if (i >= n) return;
    char *o = tmp + (size_t)i * (L + 1);
    uint8_t buf[256]; bool rev, hasN;
    if (!decode_read(seqb, seqlen, possum, noise, noisepos, nlpos, revb, nrevb, revtail, i, L, buf, &rev, &hasN, err)) {
        isN[i] = 0; for (int j = 0; j < L; j++) o[j] = 'A'; o[L] = '\n'; return;       // a line all the same: the host refuses the archive (*err)
    }
    if (!rev) for (int j = 0; j < L; j++) o[j] = "ACGTN"[buf[j]];
    else for (int j = 0; j < L; j++) { const int b = buf[L - 1 - j]; o[j] = "ACGTN"[b == 4 ? 4 : 3 - b]; }
    o[L] = '\n';
    isN[i] = hasN ? 1u : 0u;
}
// stable split of the lines: reads without N to outA[rankA], reads with N to outN[i - rankA]
__global__ void k_split_lines(const char *tmp, const uint32_t *isN, const uint32_t *rankN, uint32_t n, int L, char *outA, char *outN)
{
    const uint64_t gid = harc_gid();
    const uint64_t LL = (uint64_t)L + 1;
    if (gid >= (uint64_t)n * LL) return;
    const uint32_t i = (uint32_t)(gid / LL); const uint32_t j = (uint32_t)(gid % LL);
    const char ch = tmp[gid];
    if (isN[i]) outN[(uint64_t)rankN[i] * LL + j] = ch; else outA[(uint64_t)(i - rankN[i]) * LL + j] = ch;
}
__global__ void k_codes_to_lines(const uint8_t *codes, uint32_t n, int L, char *out)
{
    const uint64_t gid = harc_gid();
    const uint64_t LL = (uint64_t)L + 1;
    if (gid >= (uint64_t)n * LL) return;
    const uint32_t i = (uint32_t)(gid / LL); const uint32_t j = (uint32_t)(gid % LL);
    out[gid] = j == (uint32_t)L ? '\n' : "ACGT"[codes[(uint64_t)i * L + j] & 3];
}

#define G256(n) harc_grid256((uint64_t)(n)), dim3(256), 0, c->stream

// ------------------------------------------------------------------------------------------------ one shard: its streams, on the device, as lines
struct View { const uint8_t *p = nullptr; size_t n = 0; };        // host memory somebody else owns
static View view_of(const std::vector<uint8_t> &v) { return View{ v.data(), v.size() }; }
static bool get_out(harc_amd_ctx *c, int id, int shard, View *v)
{
    auto it = c->out.find(std::make_pair(id, shard));
    if (it == c->out.end()) return false;
    *v = it->second.ptr ? View{ it->second.ptr, it->second.len } : view_of(it->second.own);
    return true;
}
static int up(harc_amd_ctx *c, View h, uint8_t **d)
{
    RC_TRY(dalloc(c, d, h.n + 16));
    if (h.n) HIP_TRY(hipMemcpyAsync(*d, h.p, h.n, hipMemcpyHostToDevice, c->stream));
    return HARC_AMD_OK;
}

// the seven streams of a shard, out of the context that has just encoded them or out of output/read_*.txt.<e>
enum { S_SEQ, S_SEQ_TAIL, S_POS, S_NOISE, S_NOISEPOS, S_REV, S_REV_TAIL, S_COUNT };
struct ShardStreams { View v[S_COUNT]; std::vector<uint8_t> own[S_COUNT]; };      // own: what streams_from_files read
static int streams_from_context(harc_amd_ctx *c, int e, ShardStreams *s)
{
    static const int id[S_COUNT] = { HARC_AMD_S2_SEQ, HARC_AMD_S2_SEQ_TAIL, HARC_AMD_S2_POS, HARC_AMD_S2_NOISE, HARC_AMD_S2_NOISEPOS, HARC_AMD_S2_REV, HARC_AMD_S2_REV_TAIL };
    for (int k = 0; k < S_COUNT; k++)
        if (!get_out(c, id[k], e, &s->v[k])) { harc_set_error("shard %d streams missing", e); return HARC_AMD_ESTATE; }
    return HARC_AMD_OK;
}
static int streams_from_files(const std::string &od, int e, ShardStreams *s)
{
    static const char *const stem[S_COUNT] = { "read_seq.txt", "read_seq.txt", "read_pos.txt", "read_noise.txt", "read_noisepos.txt", "read_rev.txt", "read_rev.txt" };
    for (int k = 0; k < S_COUNT; k++) {
        const bool tail = k == S_SEQ_TAIL || k == S_REV_TAIL;
        if (!slurp_file(od + stem[k] + "." + std::to_string(e) + (tail ? ".tail" : ""), s->own[k], true)) { harc_set_error("shard %d: stream files missing", e); return HARC_AMD_EIO; }
        s->v[k] = view_of(s->own[k]);
    }
    return HARC_AMD_OK;
}

// What the decode kernels read of a shard, in the order of their arguments.  n == 0: a shard without reads, nothing to decode
struct ShardDev { uint8_t *seqb; uint64_t seqlen; uint64_t *possum; uint8_t *noise, *noisepos; uint64_t *nlpos; uint8_t *rev; uint64_t nrev; uint8_t *revtail; uint32_t n = 0; };
#define SHARD_ARGS(d) (d).seqb, (d).seqlen, (d).possum, (d).noise, (d).noisepos, (d).nlpos, (d).rev, (d).nrev, (d).revtail, (d).n
// The streams of shard e on the device: consensus unpacked to a code per byte, possum[i] = sum of the pos bytes up to read i, nlpos[i] = where the i-th '\n' of
// read_noise sits.  The streams come from outside the program: that they announce the same number of reads three times over -- a pos byte, a rev bit or tail
// byte and a line of read_noise per read, a read_noisepos byte for every other byte of read_noise -- is decided here, on the host, and the decode kernels are
// launched behind it: they index nlpos by the read and read_noisepos by (bytes of read_noise in front of the read) - (lines in front of it).
// Pool memory: the caller's PoolScope.  Synchronises the stream once
static int shard_prepare(harc_amd_ctx *c, int e, const ShardStreams &s, ShardDev *d)
{
    const View &seq = s.v[S_SEQ], &seqt = s.v[S_SEQ_TAIL], &pos = s.v[S_POS], &noise = s.v[S_NOISE], &npz = s.v[S_NOISEPOS], &rev = s.v[S_REV], &revt = s.v[S_REV_TAIL];
    d->n = 0;
    if (pos.n == 0) return HARC_AMD_OK;
    if (pos.n > 0xFFFFFFFFull || 8 * rev.n + revt.n != pos.n) { harc_set_error("shard %d: rev stream does not match pos stream", e); return HARC_AMD_EIO; }
    const uint32_t n = (uint32_t)pos.n;
    const size_t nnoise = noise.n;
    uint8_t *d_seq, *d_seqt, *d_pos; uint64_t *p64; uint32_t *fl, *rk;
    RC_TRY(up(c, seq, &d_seq)); RC_TRY(up(c, seqt, &d_seqt)); RC_TRY(up(c, pos, &d_pos)); RC_TRY(up(c, noise, &d->noise));
    RC_TRY(up(c, npz, &d->noisepos)); RC_TRY(up(c, rev, &d->rev)); RC_TRY(up(c, revt, &d->revtail));
    d->seqlen = 4 * (uint64_t)seq.n + seqt.n; d->nrev = rev.n;
    RC_TRY(dalloc(c, &d->seqb, (size_t)d->seqlen + 16)); RC_TRY(dalloc(c, &p64, (size_t)n + 1)); RC_TRY(dalloc(c, &d->possum, (size_t)n + 1));
    RC_TRY(dalloc(c, &d->nlpos, (size_t)n + 1)); RC_TRY(dalloc(c, &fl, nnoise + 1)); RC_TRY(dalloc(c, &rk, nnoise + 1));
    hipLaunchKernelGGL(k_unpack_seq, G256(d->seqlen), d_seq, (uint64_t)seq.n, d_seqt, (uint64_t)seqt.n, d->seqb);
    hipLaunchKernelGGL(k_pos_to_u64, G256(n), d_pos, n, p64);
    RC_TRY(prim_incl_scan_u64(c, p64, d->possum, n));
    // rank of every '\n' among the '\n's; one flag more, a zero, and its rank is their number
    hipLaunchKernelGGL(k_nl_flags, G256(nnoise), d->noise, (uint64_t)nnoise, fl);
    HIP_TRY(hipMemsetAsync(fl + nnoise, 0, 4, c->stream));
    RC_TRY(prim_excl_scan_u32(c, fl, rk, nnoise + 1));
    uint32_t lines = 0;
    HIP_TRY(hipMemcpyAsync(&lines, rk + nnoise, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (lines != n) { harc_set_error("shard %d: read_noise holds %u lines, read_pos %u reads", e, lines, n); return HARC_AMD_EIO; }
    if (npz.n != nnoise - n) { harc_set_error("shard %d: read_noisepos holds %zu bytes, read_noise announces %zu", e, npz.n, nnoise - n); return HARC_AMD_EIO; }
    hipLaunchKernelGGL(k_nl_positions, G256(nnoise), d->noise, rk, (uint64_t)nnoise, d->nlpos);         // (n lines: every nlpos[0 .. n) is written, none beyond)
    HIP_TRY(hipGetLastError());
    d->n = n;
    return HARC_AMD_OK;
}

// A prepared shard as text, for the two file decoders: nA lines without N in outA and nN lines with N in outN, each in stream order (decoder.cpp:110-129 routes
// the reads with N to a file of their own).  Pool memory: the caller's PoolScope.  The stream has been synchronised on return
struct ShardLines { char *outA, *outN; uint32_t nA, nN; };
static int shard_to_lines(harc_amd_ctx *c, const ShardDev &d, int L, unsigned int *d_err, ShardLines *out)
{
    const uint32_t n = d.n; const size_t LL = (size_t)L + 1;
    uint32_t *isN, *rkN; char *tmp;
    RC_TRY(dalloc(c, &isN, (size_t)n + 1)); RC_TRY(dalloc(c, &rkN, (size_t)n + 1));
    RC_TRY(dalloc(c, &tmp, (size_t)n * LL + 16)); RC_TRY(dalloc(c, &out->outA, (size_t)n * LL + 16)); RC_TRY(dalloc(c, &out->outN, (size_t)n * LL + 16));
    HIP_TRY(hipMemsetAsync(isN, 0, ((size_t)n + 1) * 4, c->stream));
    hipLaunchKernelGGL(k_decode_text, G256(n), SHARD_ARGS(d), L, tmp, isN, d_err);
    RC_TRY(prim_excl_scan_u32(c, isN, rkN, (size_t)n + 1));
    hipLaunchKernelGGL(k_split_lines, G256((uint64_t)n * LL), tmp, isN, rkN, n, L, out->outA, out->outN);
    HIP_TRY(hipMemcpyAsync(&out->nN, rkN + n, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    out->nA = n - out->nN;
    return HARC_AMD_OK;
}

// unaligned singletons, 2-bit packed + ASCII tail, L bases each (decoder.cpp:148-158): *ns of them as a code per byte, and as text lines when `lines` is given
static int singletons_unpack(harc_amd_ctx *c, View sg, View sgt, int L, uint32_t *ns, uint8_t **codes, char **lines)
{
    const uint64_t nb = 4 * (uint64_t)sg.n + sgt.n;
    *ns = (uint32_t)(nb / L);
    if (!*ns) return HARC_AMD_OK;
    uint8_t *d_sg, *d_sgt;
    RC_TRY(up(c, sg, &d_sg)); RC_TRY(up(c, sgt, &d_sgt)); RC_TRY(dalloc(c, codes, (size_t)nb + 16));
    hipLaunchKernelGGL(k_unpack_seq, G256(nb), d_sg, (uint64_t)sg.n, d_sgt, (uint64_t)sgt.n, *codes);
    if (lines) {
        RC_TRY(dalloc(c, lines, (size_t)*ns * (L + 1) + 16));
        hipLaunchKernelGGL(k_codes_to_lines, G256((uint64_t)*ns * (L + 1)), *codes, *ns, L, *lines);
    }
    return HARC_AMD_OK;
}

// the archive under <basedir>/output/ for one of the two file decoders: read length out of read_meta.txt (getDataParams, decoder.cpp:324-333), a context of its own
static int open_archive(const harc_amd_params *params, const char *basedir, int32_t num_thr_e, std::string *od, int *L, harc_amd_ctx **c)
{
    if (!params || !basedir || num_thr_e < 1) return HARC_AMD_EINVAL;
    *od = std::string(basedir) + "/output/";
    std::vector<uint8_t> meta;
    if (!slurp_file(*od + "read_meta.txt", meta, true)) { harc_set_error("cannot read %sread_meta.txt", od->c_str()); return HARC_AMD_EIO; }
    meta.push_back(0);
    *L = atoi((const char *)meta.data());
    return side_context(params, *L, c, num_thr_e);
}

extern "C" int harc_amd_reads_signature_device(harc_amd_ctx *c, const char *d_ascii, uint32_t n, uint32_t stride, uint64_t *sig3)
{
    if (!c || !sig3 || (n && !d_ascii) || stride < (uint32_t)c->P.readlen) return HARC_AMD_EINVAL;
    HIP_TRY(hipSetDevice(c->P.device));
    PoolScope scope(c);
    unsigned long long *d_sig = nullptr; RC_TRY(dalloc(c, &d_sig, 4));
    HIP_TRY(hipMemsetAsync(d_sig, 0, 32, c->stream));
    if (n) hipLaunchKernelGGL(k_sig_ascii, G256(n), d_ascii, n, stride, c->P.readlen, d_sig);
    HIP_TRY(hipMemcpyAsync(sig3, d_sig, 24, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return HARC_AMD_OK;
}

extern "C" int harc_amd_decode_signature(harc_amd_ctx *c, uint64_t *sig3)
{
    if (!c || !sig3) return HARC_AMD_EINVAL;
    if (!c->have_s2) { harc_set_error("harc_amd_decode_signature: encode first"); return HARC_AMD_ESTATE; }
    HIP_TRY(hipSetDevice(c->P.device));
    const int L = c->P.readlen;
    PoolScope scope(c);                                            // the caller's context lives on: whatever way this call ends, the pool is as it found it
    unsigned long long *d_sig = nullptr; unsigned int *d_err = nullptr;
    RC_TRY(dalloc(c, &d_sig, 4)); RC_TRY(dalloc(c, &d_err, 4));
    HIP_TRY(hipMemsetAsync(d_sig, 0, 32, c->stream)); HIP_TRY(hipMemsetAsync(d_err, 0, 16, c->stream));
    for (int e = 0; e < c->P.num_thr; e++) {
        ShardStreams s; ShardDev d;
        RC_TRY(streams_from_context(c, e, &s));
        PoolScope shard(c);
        RC_TRY(shard_prepare(c, e, s, &d));
        if (!d.n) continue;
        hipLaunchKernelGGL(k_decode_sig, G256(d.n), SHARD_ARGS(d), L, d_sig, d_err);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    {   // unaligned singletons and unaligned N reads (decoder.cpp:148-169)
        View sg, sgt, nt;
        if (!get_out(c, HARC_AMD_S2_SINGLETON, 0, &sg) || !get_out(c, HARC_AMD_S2_SINGLETON_TAIL, 0, &sgt) || !get_out(c, HARC_AMD_S2_INPUT_N, 0, &nt)) {
            harc_set_error("singleton streams missing"); return HARC_AMD_ESTATE;
        }
        uint32_t ns = 0; uint8_t *codes = nullptr, *d_nt = nullptr;
        RC_TRY(singletons_unpack(c, sg, sgt, L, &ns, &codes, nullptr));
        if (ns) hipLaunchKernelGGL(k_sig_codes, G256(ns), codes, ns, L, d_sig);
        const uint32_t nn = (uint32_t)(nt.n / (L + 1));
        if (nn) {
            RC_TRY(up(c, nt, &d_nt));
            hipLaunchKernelGGL(k_sig_ascii, G256(nn), (const char *)d_nt, nn, (uint32_t)L + 1, L, d_sig);
        }
    }
    unsigned int err = 0;
    HIP_TRY(hipMemcpyAsync(sig3, d_sig, 24, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (err) { harc_set_error("decode: %u reads with inconsistent pos/noise streams", err); return HARC_AMD_EIO; }
    return HARC_AMD_OK;
}

// The ranges of output lines a decoder writes, one after the other (./harc -d -r): [lo, hi) in lines of the whole output, `out`: the lines written in front of it.
// No range asked for: the whole output as one range
struct LineRange { uint64_t lo, hi, out; };
static int line_ranges(const char *who, int32_t n_ranges, const uint64_t *first, const uint64_t *count, uint64_t total, std::vector<LineRange> *R, uint64_t *lines_out)
{
    R->clear(); *lines_out = 0;
    if (n_ranges == 0) { R->push_back(LineRange{ 0, total, 0 }); *lines_out = total; return HARC_AMD_OK; }
    if (n_ranges < 0 || n_ranges > 2 || !first || !count) { harc_set_error("%s: one or two ranges, not %d", who, n_ranges); return HARC_AMD_EINVAL; }
    for (int r = 0; r < n_ranges; r++) {
        if (count[r] == 0 || first[r] >= total || count[r] > total - first[r]) {
            harc_set_error("%s: lines %llu .. %llu are wanted, the archive holds %llu", who, (unsigned long long)first[r] + 1, (unsigned long long)(first[r] + count[r]), (unsigned long long)total);
            return HARC_AMD_EINVAL;
        }
        R->push_back(LineRange{ first[r], first[r] + count[r], *lines_out });
        *lines_out += count[r];
    }
    return HARC_AMD_OK;
}

// decoder.out <basedir> <num_thr> <num_thr_e>  (src/decoder.cpp:44-172, harc:188): writes output/output.dna, or the lines of the ranges alone
extern "C" int harc_amd_decoder_range_files(const harc_amd_params *params, const char *basedir, int32_t num_thr_e, int32_t n_ranges, const uint64_t *first, const uint64_t *count)
{
    std::string od; int L = 0; CtxGuard guard;
    RC_TRY(open_archive(params, basedir, num_thr_e, &od, &L, &guard.c));
    harc_amd_ctx *c = guard.c;
    // output.dna holds one line per read: its length is known before a byte is decoded -- a read per byte of read_pos.txt.<e> (decoder.cpp:96), the singletons
    // (4 bases per byte + tail, :148-158), input_N.dna as it is (:166-168)
    const size_t LL = (size_t)L + 1;
    auto size_of = [&od](const std::string &name) { uint64_t n = 0; (void)file_size((od + name).c_str(), &n); return (size_t)n; };     // 0: no such regular file
    size_t total_out = size_of("input_N.dna");
    for (int e = 0; e < num_thr_e; e++) total_out += size_of("read_pos.txt." + std::to_string(e)) * LL;
    total_out += ((4 * size_of("read_singleton.txt") + size_of("read_singleton.txt.tail")) / (size_t)L) * LL;
    // the N reads of every shard come behind the singletons (decoder.cpp:159-165): they wait in device memory of their own (declared in front of the
    // drain: it goes after the drain has written what it still holds)
    struct NParts { harc_amd_ctx *c; std::vector<std::pair<char *, size_t>> v; ~NParts() { for (auto &x : v) if (x.first) harc_raw_free(c, x.first); } } nparts{ c, {} };
    std::vector<LineRange> R; uint64_t lines_out = 0;
    RC_TRY(line_ranges("decoder", n_ranges, first, count, total_out / LL, &R, &lines_out));
    const double td0 = mono_now(); double t_slurp = 0, t_put = 0;
    FileDrain drain(c);
    RC_TRY(drain.start(od + "output.dna", n_ranges ? (size_t)lines_out * LL : total_out));
    const double td1 = mono_now();
    uint64_t out_at = 0;
    // the segment of `len` bytes that continues the whole output at byte out_at, in device memory (d) or on the host (h): the parts of it inside a range are written
    auto emit = [&](const char *d, const uint8_t *h, size_t len) -> int {
        for (const LineRange &r : R) {
            const uint64_t rlo = r.lo * LL, rhi = n_ranges ? r.hi * LL : (uint64_t)total_out;     // (the whole decode: an input_N.dna that is not whole lines is written as it is)
            const uint64_t lo = out_at > rlo ? out_at : rlo, hi = out_at + len < rhi ? out_at + len : rhi;
            if (lo >= hi) continue;
            if (d) RC_TRY(drain.put(d + (lo - out_at), (size_t)(hi - lo), r.out * LL + (lo - rlo)));
            else RC_TRY(drain.put_host(h + (lo - out_at), (size_t)(hi - lo), r.out * LL + (lo - rlo)));
        }
        out_at += len;
        return HARC_AMD_OK;
    };
    unsigned int *d_err = nullptr; RC_TRY(dalloc(c, &d_err, 4));
    HIP_TRY(hipMemsetAsync(d_err, 0, 16, c->stream));
    for (int e = 0; e < num_thr_e; e++) {
        ShardStreams s; ShardDev d; ShardLines ln;
        { const double ts0 = mono_now(); RC_TRY(streams_from_files(od, e, &s)); t_slurp += mono_now() - ts0; }
        PoolScope shard(c);                                        // (the copies out of outA / outN are on the stream in front of whatever takes their place)
        RC_TRY(shard_prepare(c, e, s, &d));
        if (!d.n) continue;
        RC_TRY(shard_to_lines(c, d, L, d_err, &ln));
        const size_t bytesA = (size_t)ln.nA * LL, bytesN = (size_t)ln.nN * LL;
        if (bytesN) {
            char *keep = nullptr;
            RC_TRY(harc_raw_alloc(c, (void **)&keep, bytesN + 16));
            nparts.v.emplace_back(keep, bytesN);
            HIP_TRY(hipMemcpyAsync(keep, ln.outN, bytesN, hipMemcpyDeviceToDevice, c->stream));
        }
        { const double tp0 = mono_now(); RC_TRY(emit(ln.outA, nullptr, bytesA)); t_put += mono_now() - tp0; }
    }
    {   // singletons (decoder.cpp:148-158), then the N reads of every shard (:159-165), then input_N.dna (:166-168)
        std::vector<uint8_t> sg, sgt, nt;
        if (!slurp_file(od + "read_singleton.txt", sg, true) || !slurp_file(od + "read_singleton.txt.tail", sgt, true)) { harc_set_error("singleton files missing"); return HARC_AMD_EIO; }
        (void)slurp_file(od + "input_N.dna", nt, false);
        PoolScope scope(c);
        uint32_t ns = 0; uint8_t *codes = nullptr; char *lines = nullptr;
        RC_TRY(singletons_unpack(c, view_of(sg), view_of(sgt), L, &ns, &codes, &lines));
        if (ns) RC_TRY(emit(lines, nullptr, (size_t)ns * LL));
        for (auto &p : nparts.v) RC_TRY(emit(p.first, nullptr, p.second));
        RC_TRY(emit(nullptr, nt.data(), nt.size()));
    }
    if (out_at != total_out) { harc_set_error("decoder: %llu bytes decoded, the stream files announce %zu", (unsigned long long)out_at, total_out); return HARC_AMD_EIO; }
    unsigned int err = 0;
    HIP_TRY(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const double tf0 = mono_now();
    RC_TRY(drain.finish());
    if (getenv("HARC_AMD_TRACE")) fprintf(stderr, "[decoder] %.3f s: output mapped and ring ready %.3f, stream files read %.3f, waiting for ring slices %.3f, last slices written %.3f\n", mono_now() - td0, td1 - td0, t_slurp, t_put, mono_now() - tf0);
    if (err) { harc_set_error("decoder: %u reads with inconsistent pos/noise streams", err); return HARC_AMD_EIO; }
    printf("Decoding done\n");                                                 // decoder.cpp:170
    return HARC_AMD_OK;
}
extern "C" int harc_amd_decoder_files(const harc_amd_params *params, const char *basedir, int32_t num_thr_e)
{
    return harc_amd_decoder_range_files(params, basedir, num_thr_e, 0, nullptr, nullptr);
}

// signature of the reads the context currently holds (2-bit clean reads + 3-bit N reads): the other side of the round-trip check
// when the inputs never existed as ASCII on this GPU (the shard received through the all-to-all)
__global__ void k_sig_packed2(const uint64_t *reads, uint32_t n, int L, int W, unsigned long long *sig)
{
    const uint32_t i = harc_gid32();
    uint64_t h = READ_HASH_INIT;
    if (i < n) {
        const uint64_t *r = reads + (size_t)i * W;
        for (int j = 0; j < L; j++) { const int pc = (int)((r[j >> 5] >> (2 * (j & 31))) & 3); h = read_hash_step(h, ((pc & 1) << 1) | (pc >> 1)); }
        h = mix64(h);
    }
    sig_accumulate(h, i < n, sig);
}
__global__ void k_sig_packed3(const uint64_t *reads, uint32_t n, int L, int W3, unsigned long long *sig)
{
    const uint32_t i = harc_gid32();
    uint64_t h = READ_HASH_INIT;
    if (i < n) {
        const uint64_t *r = reads + (size_t)i * W3;
        for (int j = 0; j < L; j++) {
            const int off = 3 * j, wi = off >> 6, sh = off & 63;
            uint64_t v = r[wi] >> sh;
            if (sh > 61 && wi + 1 < W3) v |= r[wi + 1] << (64 - sh);
            const int c3 = (int)(v & 7);
            h = read_hash_step(h, c3 == 0 ? 0 : c3 == 4 ? 1 : c3 == 2 ? 2 : c3 == 6 ? 3 : 4);
        }
        h = mix64(h);
    }
    sig_accumulate(h, i < n, sig);
}
extern "C" int harc_amd_input_signature(harc_amd_ctx *c, uint64_t *sig3)
{
    if (!c || !sig3) return HARC_AMD_EINVAL;
    HIP_TRY(hipSetDevice(c->P.device));
    PoolScope scope(c);
    unsigned long long *d_sig = nullptr; RC_TRY(dalloc(c, &d_sig, 4));
    HIP_TRY(hipMemsetAsync(d_sig, 0, 32, c->stream));
    if (c->N && c->d_reads) hipLaunchKernelGGL(k_sig_packed2, G256(c->N), c->d_reads, c->N, c->P.readlen, c->W, d_sig);
    if (c->NN && c->d_nreads3) hipLaunchKernelGGL(k_sig_packed3, G256(c->NN), c->d_nreads3, c->NN, c->P.readlen, c->W3, d_sig);
    HIP_TRY(hipMemcpyAsync(sig3, d_sig, 24, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return HARC_AMD_OK;
}

// ------------------------------------------------------------------------------------------------ -p decode chain
// unpack_order.out + decoder_preserve.out + merge_N.out (harc:183-185) in one call: every read goes back to its line of the original
// FASTQ.  read_order.bin (packed, pack_order.cpp) tells the original clean-read index of every decoded clean read in stream order,
// read_order_N_pe.bin the index among the N reads of every decoded / left-over N read, read_order_N.bin the original line of every
// N read (merge_N.cpp:37-57).
__global__ void k_unpack_order(const uint32_t *packed, uint32_t ngroups, int numbits, uint32_t *out)      // unpack_order.cpp:34-62
{
    const uint64_t gid = harc_gid();
    if (gid >= (uint64_t)ngroups * 32) return;
    const uint32_t g = (uint32_t)(gid >> 5); const int k = (int)(gid & 31);
    const uint32_t *w = packed + (size_t)g * numbits;
    const int bit = k * numbits, wi = bit >> 5, sh = bit & 31;
    uint64_t v = w[wi];
    if (sh + numbits > 32) v |= (uint64_t)w[wi + 1] << 32;
    out[gid] = (uint32_t)((v >> sh) & (numbits == 32 ? 0xFFFFFFFFull : ((1ull << numbits) - 1)));
}
// line i of src goes to line order[i] - lo of dst when lo <= order[i] < hi (one bin of restore_order, decoder_preserve.cpp:246-290);
// order[i] >= ndst is an inconsistent archive
__global__ void k_permute_lines(const char *src, const uint32_t *order, uint32_t n, int L, char *dst, uint32_t lo, uint32_t hi, uint32_t ndst, unsigned int *err)
{
    const uint64_t gid = harc_gid();
    const uint64_t LL = (uint64_t)L + 1;
    if (gid >= (uint64_t)n * LL) return;
    const uint32_t i = (uint32_t)(gid / LL);
    const uint32_t o = order[i];
    if (o >= ndst) { if (gid % LL == 0) atomicAdd(err, 1u); return; }
    if (o < lo || o >= hi) return;
    dst[(uint64_t)(o - lo) * LL + gid % LL] = src[gid];
}
__global__ void k_mark_N(const uint32_t *orderN, uint32_t nN, uint32_t total, uint32_t *flag, unsigned int *err)
{
    const uint32_t m = harc_gid32();
    if (m >= nN) return;
    if (orderN[m] >= total) { atomicAdd(err, 1u); return; }
    flag[orderN[m]] = 1u;
}
// output lines [p0, p0 + n): line p is the next read with N (flag) or the next clean read; cl / nl hold the clean reads from index clo on and
// the N reads from index nlo on (merge_N.cpp:37-57, one bin of it)
__global__ void k_merge_lines(const char *clean, const char *withN, const uint32_t *flag, const uint32_t *rankN, uint32_t p0, uint32_t n, uint32_t clo, uint32_t nlo, int L, char *out)
{
    const uint64_t gid = harc_gid();
    const uint64_t LL = (uint64_t)L + 1;
    if (gid >= (uint64_t)n * LL) return;
    const uint32_t p = p0 + (uint32_t)(gid / LL); const uint64_t j = gid % LL;
    out[gid] = flag[p] ? withN[(uint64_t)(rankN[p] - nlo) * LL + j] : clean[(uint64_t)(p - rankN[p] - clo) * LL + j];
}

extern "C" int harc_amd_decoder_preserve_range_files(const harc_amd_params *params, const char *basedir, int32_t num_thr_e, int32_t n_ranges, const uint64_t *first, const uint64_t *count)
{
    std::string od; int L = 0; CtxGuard guard;
    RC_TRY(open_archive(params, basedir, num_thr_e, &od, &L, &guard.c));
    harc_amd_ctx *c = guard.c;
    std::vector<uint8_t> pord, ptail, ordNpe, ordN;
    if (!slurp_file(od + "read_order.bin", pord, true) || !slurp_file(od + "read_order.bin.tail", ptail, true) || !slurp_file(od + "read_order_N_pe.bin", ordNpe, true) ||
        !slurp_file(od + "read_order_N.bin", ordN, true)) { harc_set_error("order files missing: was the archive made with -p?"); return HARC_AMD_EIO; }
    const size_t LL = (size_t)L + 1;
    // ---- unpack_order
    uint32_t nC = 0; int numbits = 0;
    if (pord.size() >= 8) { memcpy(&numbits, pord.data(), 4); memcpy(&nC, pord.data() + 4, 4); }
    const uint32_t ng = nC / 32, ntail = nC % 32;
    if (nC && (numbits < 1 || numbits > 32 || pord.size() != 8 + (size_t)ng * numbits * 4 || ptail.size() != (size_t)ntail * 4)) { harc_set_error("read_order.bin is not a pack_order file"); return HARC_AMD_EIO; }
    const uint32_t nN = (uint32_t)(ordN.size() / 4);
    if (ordNpe.size() != ordN.size()) { harc_set_error("read_order_N_pe.bin and read_order_N.bin disagree"); return HARC_AMD_EIO; }
    const uint64_t total64 = (uint64_t)nC + nN;
    if (total64 > 4294967290ull) { harc_set_error("more than 4294967290 reads"); return HARC_AMD_EINVAL; }
    const uint32_t total = (uint32_t)total64;
    std::vector<LineRange> R; uint64_t lines_out = 0;
    RC_TRY(line_ranges("decoder -p", n_ranges, first, count, total64, &R, &lines_out));
    uint32_t *d_order = nullptr, *d_ordNpe = nullptr, *d_ordN = nullptr, *flag = nullptr, *rankN = nullptr; unsigned int *d_err = nullptr;
    RC_TRY(dalloc(c, &d_order, (size_t)nC + 32)); RC_TRY(dalloc(c, &d_ordNpe, (size_t)nN + 1)); RC_TRY(dalloc(c, &d_ordN, (size_t)nN + 1)); RC_TRY(dalloc(c, &d_err, 4));
    RC_TRY(dalloc(c, &flag, (size_t)total + 1)); RC_TRY(dalloc(c, &rankN, (size_t)total + 1));
    HIP_TRY(hipMemsetAsync(d_err, 0, 16, c->stream));
    if (ng) {
        PoolScope scope(c);
        uint8_t *d_p = nullptr; RC_TRY(up(c, View{ pord.data() + 8, (size_t)ng * numbits * 4 }, &d_p));
        hipLaunchKernelGGL(k_unpack_order, G256((uint64_t)ng * 32), (const uint32_t *)d_p, ng, numbits, d_order);
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (ntail) HIP_TRY(hipMemcpyAsync(d_order + (size_t)ng * 32, ptail.data(), (size_t)ntail * 4, hipMemcpyHostToDevice, c->stream));
    if (nN) { HIP_TRY(hipMemcpyAsync(d_ordNpe, ordNpe.data(), (size_t)nN * 4, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_ordN, ordN.data(), (size_t)nN * 4, hipMemcpyHostToDevice, c->stream)); }
    // which output lines are reads with N (merge_N.cpp:37-57), and how many of those come before each line
    HIP_TRY(hipMemsetAsync(flag, 0, ((size_t)total + 1) * 4, c->stream));
    if (nN) hipLaunchKernelGGL(k_mark_N, G256(nN), d_ordN, nN, total, flag, d_err);
    RC_TRY(prim_excl_scan_u32(c, flag, rankN, (size_t)total + 1));
    HIP_TRY(hipStreamSynchronize(c->stream));
    pord.clear(); pord.shrink_to_fit();

    // ---- bins of output lines.  The reference restores the order through host memory in bins of MAX_BIN_SIZE * 2e8 / 7 reads (-m,
    // decoder_preserve.cpp:249-253), reading the decoded reads of every bin back from a temporary file; here a bin is what fits in HBM next
    // to the scratch of one shard's decode (and no more than -m asks for), and every bin decodes the streams again and keeps the lines that
    // fall into it -- decoding is cheap, no temporary file, host memory bounded by one output chunk.
    uint64_t bin_lines;
    {
        const int mgb = c->P.decode_memory_gb > 3 ? c->P.decode_memory_gb : (c->P.decode_memory_gb == 0 ? 7 : 3);     // harc:225 default 7; decoder_preserve.cpp:249-252
        bin_lines = (uint64_t)mgb * 200000000ull / 7ull;
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
            fr += c->pool_total;
            // every bin decodes every shard in full: the scratch of the LARGEST shard (three line buffers + streams + scans, ~3 (L+1) + 64
            // bytes per read of the shard) is needed whatever the bin size, and is taken off before the bin gets its quarter
            uint64_t nmax = 0;
            for (int e = 0; e < num_thr_e; e++) {
                uint64_t sz = 0;
                if (file_size((od + "read_pos.txt." + std::to_string(e)).c_str(), &sz) && sz > nmax) nmax = sz;
            }
            const double shard_scratch = (double)nmax * (3.0 * (double)LL + 64.0);
            if (shard_scratch > 0.9 * (double)fr) {
                harc_set_error("decoder_preserve: the largest shard (%llu reads) needs %.1f GB of decode scratch, %.1f GB are free; compress with more threads (-t) for smaller shards",
                               (unsigned long long)nmax, shard_scratch / 1e9, (double)fr / 1e9);
                return HARC_AMD_ENOMEM;
            }
            const uint64_t cap = (uint64_t)(0.25 * ((double)fr - shard_scratch) / (double)(3 * LL));     // clean + N + merged lines of the bin: a quarter of what is left
            if (bin_lines > (cap ? cap : 1)) bin_lines = cap ? cap : 1;
        }
        if (const char *e = getenv("HARC_AMD_BIN_READS")) bin_lines = strtoull(e, nullptr, 10);      // tests: tiny bins
        if (bin_lines < 1) bin_lines = 1;
    }
    FILE *fo = fopen((od + "output.dna").c_str(), "wb");
    if (!fo) { harc_set_error("cannot create %soutput.dna", od.c_str()); return HARC_AMD_EIO; }
    struct FClose { FILE *f; ~FClose() { if (f) fclose(f); } } fcl{ fo };
    std::vector<uint8_t> sg, sgt, nt;                             // singletons and unaligned N reads: read once
    if (!slurp_file(od + "read_singleton.txt", sg, true) || !slurp_file(od + "read_singleton.txt.tail", sgt, true)) { harc_set_error("singleton files missing"); return HARC_AMD_EIO; }
    (void)slurp_file(od + "input_N.dna", nt, false);
    // what the kernels have counted into d_err so far refuses the archive
    auto refuse_counted = [&]() -> int {
        unsigned int err = 0;
        HIP_TRY(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (err) { harc_set_error("decoder -p: %u inconsistent order / stream entries", err); return HARC_AMD_EIO; }
        return HARC_AMD_OK;
    };
    // a bin is [p0, p0 + pn) inside one range (an archive without reads: one bin without lines, for the checks)
    for (const LineRange &rg : R) for (uint64_t p0 = rg.lo; p0 < rg.hi || (rg.hi == 0 && p0 == 0); p0 += bin_lines) {
        PoolScope bin(c);                                         // what a bin allocates goes with it
        const uint32_t pn = (uint32_t)(rg.hi - p0 < bin_lines ? rg.hi - p0 : bin_lines);
        uint32_t r0 = 0, r1 = 0;
        HIP_TRY(hipMemcpyAsync(&r0, rankN + p0, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(&r1, rankN + p0 + pn, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const uint32_t nlo = r0, nhi = r1, clo = (uint32_t)p0 - r0, chi = (uint32_t)(p0 + pn) - r1;     // the clean reads and the N reads of this bin
        char *clp = nullptr, *nlp = nullptr;
        RC_TRY(dalloc(c, &clp, (size_t)(chi - clo) * LL + 16)); RC_TRY(dalloc(c, &nlp, (size_t)(nhi - nlo) * LL + 16));
        // ---- decode every shard (stream order) and keep the lines of this bin: restore_order (decoder_preserve.cpp:246-290) and
        //      restore_order_N (:212-244)
        uint64_t cA = 0, cN = 0;
        for (int e = 0; e < num_thr_e; e++) {
            ShardStreams s; ShardDev d; ShardLines ln;
            RC_TRY(streams_from_files(od, e, &s));
            PoolScope shard(c);
            RC_TRY(shard_prepare(c, e, s, &d));
            if (!d.n) continue;
            RC_TRY(shard_to_lines(c, d, L, d_err, &ln));
            if (cA + ln.nA > nC || cN + ln.nN > nN) { harc_set_error("streams hold more reads than the order files"); return HARC_AMD_EIO; }
            if (ln.nA) hipLaunchKernelGGL(k_permute_lines, G256((uint64_t)ln.nA * LL), ln.outA, d_order + cA, ln.nA, L, clp, clo, chi, nC, d_err);
            if (ln.nN) hipLaunchKernelGGL(k_permute_lines, G256((uint64_t)ln.nN * LL), ln.outN, d_ordNpe + cN, ln.nN, L, nlp, nlo, nhi, nN, d_err);
            HIP_TRY(hipStreamSynchronize(c->stream));
            cA += ln.nA; cN += ln.nN;
        }
        RC_TRY(refuse_counted());                                 // (in front of the counts below: a read that could not be decoded is a line without N, whatever it was)
        {   // singletons, then the N reads that were not aligned (decoder_preserve.cpp:160-197)
            PoolScope scope(c);
            uint32_t ns = 0; uint8_t *codes = nullptr; char *sl = nullptr;
            RC_TRY(singletons_unpack(c, view_of(sg), view_of(sgt), L, &ns, &codes, &sl));
            const uint32_t nu = (uint32_t)(nt.size() / LL);
            if (cA + ns != nC || cN + nu != nN) { harc_set_error("read counts do not add up: clean %llu+%u vs %u, N %llu+%u vs %u", (unsigned long long)cA, ns, nC, (unsigned long long)cN, nu, nN); return HARC_AMD_EIO; }
            if (ns) hipLaunchKernelGGL(k_permute_lines, G256((uint64_t)ns * LL), sl, d_order + cA, ns, L, clp, clo, chi, nC, d_err);
            if (nu) {
                uint8_t *d_nt; RC_TRY(up(c, View{ nt.data(), (size_t)nu * LL }, &d_nt));
                hipLaunchKernelGGL(k_permute_lines, G256((uint64_t)nu * LL), (const char *)d_nt, d_ordNpe + cN, nu, L, nlp, nlo, nhi, nN, d_err);
            }
        }
        RC_TRY(refuse_counted());
        // ---- merge_N for the lines of the bin, written in pieces of at most 256 MiB
        const uint32_t piece = (uint32_t)(((size_t)256 << 20) / LL);
        char *outl = nullptr; RC_TRY(dalloc(c, &outl, (size_t)piece * LL + 16));
        std::vector<uint8_t> host;
        for (uint32_t q = 0; q < pn; q += piece) {
            const uint32_t m = pn - q < piece ? pn - q : piece;
            hipLaunchKernelGGL(k_merge_lines, G256((uint64_t)m * LL), clp, nlp, flag, rankN, (uint32_t)p0 + q, m, clo, nlo, L, outl);
            host.resize((size_t)m * LL);
            HIP_TRY(hipMemcpyAsync(host.data(), outl, host.size(), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (fwrite(host.data(), 1, host.size(), fo) != host.size()) { harc_set_error("short write on output.dna"); return HARC_AMD_EIO; }
        }
    }
    printf("Decoding done\n");
    return HARC_AMD_OK;
}
extern "C" int harc_amd_decoder_preserve_files(const harc_amd_params *params, const char *basedir, int32_t num_thr_e)
{
    return harc_amd_decoder_preserve_range_files(params, basedir, num_thr_e, 0, nullptr, nullptr);
}
