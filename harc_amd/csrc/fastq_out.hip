// fastq_out.hip -- the way back to FASTQ (./harc -d -q): the three files a -c -q run took the FASTQ apart into -- one id per line, one read per line, one
// quality string per line -- become 4-line records again, on the GPU.  Record i of the output is
//     id_i \n read_i \n + \n quality_i \n
// The third line is a bare '+', or -- under the rule `same` of third.h, which -c -q records in the archive member read.third when every third line of the input
// repeated its id -- '+' followed by id_i[1..].  Any other text behind the '+' of the input is not kept and cannot be restored.
//
// A streaming kernel: B bytes in, B bytes out, its floor is a device-to-device copy.  It is OUTPUT-centric.  A workgroup owns one 16-byte-aligned tile of
// FQ_TILE output bytes; it finds the first record that reaches into the tile by binary search on out_off[i] = id_start[i] + i * (2 * readlen + 4) (the line
// index of the id text is the only index there is: reads and quality values have a fixed stride), its waves take the records of the tile round robin and
// build an image of the tile in LDS, and the image leaves with one aligned 16-byte store per lane.  A lane of the wave that copies a record owns one aligned
// DWORD of the image: it fetches the (up to two) aligned source dwords that hold its four bytes from whichever of id / read / quality they come from, shifts them
// into place (v_alignbyte) and writes the dword; only a dword that a record shares with its neighbour (another wave's) is written byte by byte.  A record
// longer than a tile (an id of 40 000 bytes) is simply clipped to the tile by every workgroup it reaches into.  The first and the last 16 bytes of the whole
// output, where the caller's buffer is not aligned or does not end on a 16-byte boundary, are stored byte by byte by the lanes that hold them.
// The same lanes check the fixed-width inputs on the way -- a newline at every (readlen + 1)-stride position and nowhere else -- into an error counter.
// The plumbing of the file call (probes, guards, ring split, device buffers, kernel timer, the walk over the id file in whole lines) is fileio.h's.
#include "devutil.h"
#include "fileio.h"
#include "deflate_member.h"
#include "idmate.h"
#include "third.h"

#define FQ_TILE 16384
#define FQ_WAVES 4

// The part of the image dword at tile byte p that comes from a source segment: the segment's bytes go to tile bytes [d0, d0 + len), src is its first byte.
// Returns the bytes in place (others zero), *mask has 0xFF for each.  An aligned source dword is fetched only when one of the bytes asked for lies in it.
__device__ __forceinline__ uint32_t fq_seg(const char *src, int64_t d0, int64_t len, int64_t p, uint32_t *mask)
{
    const int64_t a = d0 - p, b = d0 + len - p;                   // the segment in the dword's own coordinates
    const int k0 = a > 0 ? (a < 4 ? (int)a : 4) : 0, k1 = b < 4 ? (b > 0 ? (int)b : 0) : 4;
    if (k0 >= k1) { *mask = 0; return 0; }
    const uintptr_t u = (uintptr_t)src + (uintptr_t)(p - d0);    // where byte 0 of the dword comes from (in front of src when k0 > 0: not fetched)
    const int sh = (int)(u & 3);
    const uint32_t *w = (const uint32_t *)(u - (uintptr_t)sh);
    uint32_t lo = 0, hi = 0;                                      // w[0] holds bytes [-sh, 4 - sh) of the dword, w[1] bytes [4 - sh, 8 - sh)
    if (k0 < 4 - sh) lo = w[0];
    if (k1 > 4 - sh) hi = w[1];
    const uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)sh);
    const uint32_t m = (k1 == 4 ? 0xFFFFFFFFu : ((1u << (8 * k1)) - 1u)) & ~((1u << (8 * k0)) - 1u);
    *mask = m;
    return v & m;
}
// bytes of a fixed-width line (L characters and a newline, at tile bytes [d0, d0 + L + 1)) in the dword at p that break the stride: a newline that is not the
// line's last byte, or a last byte that is no newline
__device__ __forceinline__ uint32_t fq_stride_errors(uint32_t v, uint32_t m, int64_t d0, int L, int64_t p)
{
    const int64_t knl = d0 + L - p;                               // where the newline belongs, in the dword's coordinates
    uint32_t bad = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const bool mine = (m >> (8 * k)) & 1u, isnl = ((v >> (8 * k)) & 0xFFu) == (uint32_t)'\n';
        bad += (mine && isnl != (knl == (int64_t)k)) ? 1u : 0u;
    }
    return bad;
}
__device__ __forceinline__ void fq_const(char ch, int64_t at, int64_t p, uint32_t *v, uint32_t *m)
{
    const int64_t k = at - p;
    if (k >= 0 && k < 4) { *v |= (uint32_t)(uint8_t)ch << (8 * (int)k); *m |= 0xFFu << (8 * (int)k); }
}

// Tile t holds the output bytes whose ADDRESS, counted from the 16-byte boundary at or below out, lies in [t * FQ_TILE, (t + 1) * FQ_TILE): `mis` = out & 15.
// nls: the line index of the id text (build_line_index; nls[-1] = -1).  err[0] / err[1]: stride errors of the reads / the quality values.
// SAME (the third lines repeat the ids): record i takes 2 * (idlen_i + 1) + 2 * readlen + 2 bytes and starts at 2 * id_start[i] + i * (2 * readlen + 2) -- still
// closed-form; the second id is one more segment from the same source line, a byte further on, behind a constant '+'.  err[2]: id lines of length 0, which no
// third line can repeat (counted where the record starts).  Without SAME the kernel is the code it was.
template <bool SAME> __global__ __launch_bounds__(64 * FQ_WAVES) void k_fq_tiles(const char *ids, const uint64_t *nls, const char *dna, const char *qual, uint32_t n, int L,
                                                            char *out, uint64_t total, uint32_t mis, uint64_t ntiles, unsigned int *err)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[FQ_TILE / 4];
    __shared__ uint32_t s_first;
    const uint64_t t = harc_bid();
    if (t >= ntiles) return;
    const uint64_t K = 2ull * (uint64_t)L + (SAME ? 2 : 4), LL = (uint64_t)L + 1, M = SAME ? 2 : 1;       // record i starts at M * id_start[i] + i * K
    const int64_t v0 = (int64_t)(t * FQ_TILE);                    // first byte of the tile, counted from the aligned boundary
    if (threadIdx.x == 0) {
        // the last record that starts at or in front of the tile's first output byte
        const uint64_t o0 = v0 > (int64_t)mis ? (uint64_t)v0 - mis : 0;
        uint64_t lo = 0, hi = (uint64_t)n - 1;
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) >> 1;
            if (M * (nls[(int64_t)mid - 1] + 1) + mid * K <= o0) lo = mid; else hi = mid - 1;
        }
        s_first = (uint32_t)lo;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t errR = 0, errQ = 0, errI = 0;
    uint8_t *tile8 = (uint8_t *)tile;
    for (uint64_t i = (uint64_t)s_first + wave; i < (uint64_t)n; i += FQ_WAVES) {
        const uint64_t ids0 = nls[(int64_t)i - 1] + 1, idlen = nls[i] - ids0;
        const int64_t b = (int64_t)(M * ids0 + i * K) + (int64_t)mis - v0;   // the record in the tile's coordinates: [b, e)
        if (b >= FQ_TILE) break;
        const int64_t e = b + (int64_t)(M * (idlen + 1) + K);        // id and its newline (SAME: twice), then the bytes every record has
        const int64_t clo = b > 0 ? b : 0, chi = e < FQ_TILE ? e : FQ_TILE;
        const int64_t d_read = b + (int64_t)idlen + 1, d_plus = d_read + (int64_t)LL, d_qual = d_plus + (SAME ? (int64_t)idlen + 1 : 2);
        if (SAME && idlen == 0 && b >= 0 && lane == 0) errI++;
        const char *s_id = ids + ids0, *s_read = dna + i * LL, *s_qual = qual + i * LL;
        for (int64_t j = (clo >> 2) + lane; j < ((chi + 3) >> 2); j += 64) {
            const int64_t p = 4 * j;
            uint32_t m0, m1, m2;
            uint32_t v = fq_seg(s_id, b, (int64_t)idlen, p, &m0);
            const uint32_t vr = fq_seg(s_read, d_read, (int64_t)LL, p, &m1);      // the line's own newline comes with it
            const uint32_t vq = fq_seg(s_qual, d_qual, (int64_t)LL, p, &m2);
            if (m1) errR += fq_stride_errors(vr, m1, d_read, L, p);
            if (m2) errQ += fq_stride_errors(vq, m2, d_qual, L, p);
            v |= vr | vq;
            uint32_t m = m0 | m1 | m2;
            fq_const('\n', d_read - 1, p, &v, &m);
            fq_const('+', d_plus, p, &v, &m);
            if (SAME) {                                           // id[1..] behind the '+'
                uint32_t m3;
                v |= fq_seg(s_id + 1, d_plus + 1, (int64_t)idlen - 1, p, &m3);
                m |= m3;
            }
            fq_const('\n', d_qual - 1, p, &v, &m);
            if (m == 0xFFFFFFFFu) tile[j] = v;                    // p >= 0 and p + 4 <= FQ_TILE: all four bytes are this record's and inside the tile
            else {
#pragma unroll
                for (int k = 0; k < 4; k++) if ((m >> (8 * k)) & 1u) tile8[p + k] = (uint8_t)(v >> (8 * k));      // (m never covers a byte outside [clo, chi))
            }
        }
    }
    if (errR) atomicAdd(&err[0], errR);
    if (errQ) atomicAdd(&err[1], errQ);
    if (SAME && errI) atomicAdd(&err[2], errI);
    __syncthreads();
    char *gbase = out - mis;
    const int64_t vlo = (int64_t)mis, vhi = (int64_t)mis + (int64_t)total;       // the output's bytes, counted from the aligned boundary
    for (int ch = threadIdx.x; ch < FQ_TILE / 16; ch += 64 * FQ_WAVES) {
        const int64_t g = v0 + 16 * (int64_t)ch;
        if (g >= vlo && g + 16 <= vhi) *(uint4 *)(gbase + g) = ((const uint4 *)tile)[ch];
        else if (g + 16 > vlo && g < vhi) {                       // the ragged head or tail of the whole output
            for (int k = 0; k < 16; k++) if (g + k >= vlo && g + k < vhi) gbase[g + k] = (char)tile8[16 * ch + k];
        }
    }
}
// the stride check alone (d_out == NULL): 16 bytes per thread of n lines of L characters and a newline
__global__ void k_fq_stride_check(const char *txt, uint64_t nbytes, int L, unsigned int *err)
{
    const uint64_t at = harc_gid() * 16;
    if (at >= nbytes) return;
    const uint64_t LL = (uint64_t)L + 1;
    uint32_t q = (uint32_t)(at % LL), bad = 0;
    for (int k = 0; k < 16 && at + k < nbytes; k++) {
        bad += ((txt[at + k] == '\n') != (q == (uint32_t)L)) ? 1u : 0u;
        if (++q == (uint32_t)LL) q = 0;
    }
    if (bad) atomicAdd(err, bad);
}

// id lines of length 0 among lines [0, n) (the validating device call under the rule same)
__global__ void k_fq_empty_ids(const uint64_t *nls, uint32_t n, unsigned int *err)
{
    const uint32_t i = harc_gid32();
    if (i < n && nls[i] == nls[(int64_t)i - 1] + 1) atomicAdd(err, 1u);
}
// what n records behind `id_bytes` bytes of id text take (a last line without its newline already counted in)
static inline uint64_t fq_text_bytes(int32_t third, uint64_t id_bytes, uint64_t n, int L)
{
    return third == TH_SAME ? 2 * id_bytes + n * (2ull * (uint64_t)L + 2) : id_bytes + n * (2ull * (uint64_t)L + 4);
}
static int fq_check_third(const char *who, int32_t third)
{
    if (third >= TH_DROPPED && third <= TH_SAME) return HARC_AMD_OK;
    harc_set_error("%s: %d is no rule of the third lines (0 dropped, 1 bare, 2 same)", who, (int)third);
    return HARC_AMD_EINVAL;
}
// n records -> d_out[0 .. total), enqueued on the context's stream; d_err[0..1] count the stride errors, d_err[2] the empty id lines under the rule same
// (third: TH_SAME, or anything else for a bare '+')
static int fq_run(harc_amd_ctx *c, const char *d_ids, const uint64_t *nls, const char *d_dna, const char *d_quality, uint32_t n, int L, char *d_out, uint64_t total,
                  unsigned int *d_err, int32_t third)
{
    if (n == 0 || total == 0) return HARC_AMD_OK;
    const uint32_t mis = (uint32_t)((uintptr_t)d_out & 15);
    const uint64_t ntiles = (mis + total + FQ_TILE - 1) / FQ_TILE;
    if (third == TH_SAME) hipLaunchKernelGGL(k_fq_tiles<true>, harc_fold256(ntiles), dim3(64 * FQ_WAVES), 0, c->stream, d_ids, nls, d_dna, d_quality, n, L, d_out, total, mis, ntiles, d_err);
    else hipLaunchKernelGGL(k_fq_tiles<false>, harc_fold256(ntiles), dim3(64 * FQ_WAVES), 0, c->stream, d_ids, nls, d_dna, d_quality, n, L, d_out, total, mis, ntiles, d_err);
    HIP_TRY(hipGetLastError());
    return HARC_AMD_OK;
}
static int fq_check_errors(harc_amd_ctx *c, const unsigned int *d_err, int L)
{
    unsigned int err[3] = { 0, 0, 0 };
    HIP_TRY(hipMemcpyAsync(err, d_err, 12, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (err[2]) {
        harc_set_error("fastq_assemble: %u id lines are empty, and no third line can repeat an empty id: the id text is damaged or another rule of the third lines was recorded than the one that held", err[2]);
        return HARC_AMD_EINVAL;
    }
    if (err[0] || err[1]) {
        harc_set_error("fastq_assemble: the fixed-width inputs are not lines of %d characters: %u bytes of the reads and %u bytes of the quality values are a newline off the %d-byte stride or no newline on it",
                       L, err[0], err[1], L + 1);
        return HARC_AMD_EINVAL;
    }
    return HARC_AMD_OK;
}

extern "C" int harc_amd_fastq_assemble_device(harc_amd_ctx *c, const char *d_ids, uint64_t id_bytes, const char *d_dna, const char *d_quality, uint32_t n_records,
                                              int32_t readlen, char *d_out, uint64_t out_capacity, uint64_t *n_out)
{
    return harc_amd_fastq_assemble_third_device(c, d_ids, id_bytes, d_dna, d_quality, n_records, readlen, d_out, out_capacity, n_out, TH_BARE);
}
extern "C" int harc_amd_fastq_assemble_third_device(harc_amd_ctx *c, const char *d_ids, uint64_t id_bytes, const char *d_dna, const char *d_quality, uint32_t n_records,
                                                    int32_t readlen, char *d_out, uint64_t out_capacity, uint64_t *n_out, int32_t third)
{
    RC_TRY(fq_check_third("fastq_assemble_device", third));
    if (!c || !n_out || readlen < 1 || readlen > 255 || (id_bytes && !d_ids) || (n_records && (!d_dna || !d_quality))) { harc_set_error("fastq_assemble_device: bad arguments"); return HARC_AMD_EINVAL; }
    HIP_TRY(hipSetDevice(c->P.device));
    PoolScope scope(c);
    const uint64_t *nls = nullptr; uint64_t lines = 0; bool open_tail = false;
    RC_TRY(text_line_index(c, d_ids, id_bytes, &nls, &lines, &open_tail));
    if (lines != (uint64_t)n_records) { harc_set_error("fastq_assemble_device: the id text holds %llu lines, %u records were announced", (unsigned long long)lines, n_records); return HARC_AMD_EINVAL; }
    const uint64_t total = fq_text_bytes(third, id_bytes + (open_tail ? 1 : 0), n_records, readlen);
    *n_out = total;
    unsigned int *d_err = nullptr; RC_TRY(dalloc(c, &d_err, 4));
    HIP_TRY(hipMemsetAsync(d_err, 0, 16, c->stream));
    if (!d_out) {
        const uint64_t nb = (uint64_t)n_records * ((uint64_t)readlen + 1);
        if (nb) {
            hipLaunchKernelGGL(k_fq_stride_check, harc_grid256((nb + 15) / 16), dim3(256), 0, c->stream, d_dna, nb, (int)readlen, d_err);
            hipLaunchKernelGGL(k_fq_stride_check, harc_grid256((nb + 15) / 16), dim3(256), 0, c->stream, d_quality, nb, (int)readlen, d_err + 1);
            if (third == TH_SAME) hipLaunchKernelGGL(k_fq_empty_ids, harc_grid256(n_records), dim3(256), 0, c->stream, nls, n_records, d_err + 2);
            HIP_TRY(hipGetLastError());
        }
        return fq_check_errors(c, d_err, readlen);
    }
    if (out_capacity < total) { harc_set_error("fastq_assemble_device: the records take %llu bytes, the buffer holds %llu", (unsigned long long)total, (unsigned long long)out_capacity); return HARC_AMD_EINVAL; }
    if (!getenv("HARC_AMD_TRACE")) {
        RC_TRY(fq_run(c, d_ids, nls, d_dna, d_quality, n_records, readlen, d_out, total, d_err, third));
        return fq_check_errors(c, d_err, readlen);
    }
    double seconds = 0;                                           // the tile kernel alone, for tools/fastq_out_rate.py
    KernelTimer timer(&seconds);
    RC_TRY(timer.begin(c->stream));
    RC_TRY(fq_run(c, d_ids, nls, d_dna, d_quality, n_records, readlen, d_out, total, d_err, third));
    RC_TRY(timer.end_mark(c->stream));
    const int rc = fq_check_errors(c, d_err, readlen);
    RC_TRY(timer.end_wait());
    const double ms = 1e3 * seconds;
    fprintf(stderr, "[fastq_out] device call: %llu bytes, tile kernel %.3f ms (%.1f GB/s of output)\n", (unsigned long long)total, ms, ms > 0 ? 1e-6 * (double)total / ms : 0.0);
    return rc;
}

// ------------------------------------------------------------------------------------------------ the files
extern "C" int harc_amd_fastq_assemble_files(const harc_amd_params *params, const char *dna_path, const char *id_path, const char *quality_path, const char *out_path)
{
    return harc_amd_fastq_assemble_files_ex(params, dna_path, id_path, quality_path, out_path, 0);
}

// what a file call knows about its three inputs before a device is touched: the read length is the length of the first read, everything else about the sizes follows from it
struct FqInputs { const char *dna_path, *id_path, *quality_path; uint64_t isz = 0, n = 0; int L = 1; bool id_open_tail = false; };
static int fq_probe(const char *who, const char *dna_path, const char *id_path, const char *quality_path, FqInputs *in)
{
    uint64_t dsz = 0, isz = 0, qsz = 0;
    if (!file_size(dna_path, &dsz)) { harc_set_error("cannot open %s", dna_path); return HARC_AMD_EIO; }
    if (!file_size(id_path, &isz)) { harc_set_error("cannot open %s", id_path); return HARC_AMD_EIO; }
    if (!file_size(quality_path, &qsz)) { harc_set_error("cannot open %s", quality_path); return HARC_AMD_EIO; }
    uint32_t L1 = 1; bool id_closed = true;
    if (dsz) RC_TRY(first_line_length(dna_path, who, &L1));
    if (isz) RC_TRY(last_byte_is_newline(id_path, &id_closed));
    const int L = (int)L1;
    const uint64_t LL = (uint64_t)L + 1;
    if (dsz % LL) { harc_set_error("%s: %s holds %llu bytes, no multiple of the %llu bytes of a read of %d characters and its newline", who, dna_path, (unsigned long long)dsz, (unsigned long long)LL, L); return HARC_AMD_EINVAL; }
    if (qsz != dsz) { harc_set_error("%s: %s holds %llu bytes and %s %llu: not a quality line per read", who, quality_path, (unsigned long long)qsz, dna_path, (unsigned long long)dsz); return HARC_AMD_EINVAL; }
    if (dsz / LL > 4294967290ull) { harc_set_error("Too many reads. HARC supports at most 4294967290 reads"); return HARC_AMD_EINVAL; }
    in->dna_path = dna_path; in->id_path = id_path; in->quality_path = quality_path;
    in->isz = isz; in->n = dsz / LL; in->L = L; in->id_open_tail = !id_closed;
    return HARC_AMD_OK;
}

// One output file: records [rec_base, rec_base + nrec) of the two fixed-stride files, with the id lines that start at byte id_begin of the id file.  The id lines
// run to the end of the id file and must be nrec -- or, with stop_at_nrec, end after exactly nrec of them: a piece is cut at that line, not only at its last
// newline, and the size of the output is only bounded beforehand.  rule (idmate.h): IDM_SLASH and IDM_SPACE patch the whole lines of every piece in front of
// the tile kernel (what is carried stays unpatched until it is a whole line); a line without the '1' to patch fails the call.  *id_end: the byte of the id file
// behind the last line taken.  on_mismatch(id lines seen) sets the error of a line count that is not nrec.
// bgzf: every assembled piece is deflated where it sits (bgzf_out.hip).  Members are cut at multiples of DM_TEXT of the whole text: what a piece leaves behind its
// last full member stays at the front of the text buffer and the next piece is assembled behind it, so the file does not depend on how the job was cut into pieces.
// Three feeders (ids, reads, quality values) and the drain are alive at the same time and the context has ONE pinned ring: gq[0 .. 4) are its four quarters --
// 0: the id feeder, 1: the read feeder, 2: the quality feeder, 3: the drain.  The caller guards the output file (OutFileGuard) and owns the context.
template <class M> static int fq_assemble_part(harc_amd_ctx *c, const RingGeom *gq, const FqInputs &in, uint64_t id_begin, uint64_t rec_base, uint64_t nrec, bool stop_at_nrec,
                                               int32_t rule, int32_t third, const char *out_path, int32_t bgzf, uint64_t *id_end, M &&on_mismatch)
{
    const int L = in.L; const uint64_t isz = in.isz;
    const uint64_t LL = (uint64_t)L + 1;
    const bool id_open_tail = in.id_open_tail && isz > id_begin;
    const uint64_t out_size = fq_text_bytes(third, (isz - id_begin) + (id_open_tail ? 1 : 0), nrec, L);    // known before a byte is read: the output is sized and mapped up front (stop_at_nrec: a bound)
    DevBuf dna{ c }, qual{ c }, out{ c }, gz{ c };
    const bool tlog = getenv("HARC_AMD_TRACE") != nullptr;
    double t_kernel = 0, t_read = 0, t_write = 0;
    KernelTimer timer(&t_kernel);
    PoolScope scope(c);
    unsigned int *d_err = nullptr; RC_TRY(dalloc(c, &d_err, 4));
    unsigned long long *d_bad = nullptr; RC_TRY(dalloc(c, &d_bad, 2));
    HIP_TRY(hipMemsetAsync(d_err, 0, 16, c->stream)); HIP_TRY(hipMemsetAsync(d_bad, 0, 16, c->stream));
    FileDrain drain(c);
    RC_TRY(drain.start(out_path, bgzf ? (size_t)dm_bound(out_size) : (size_t)out_size, &gq[3], bgzf != 0 || stop_at_nrec));
    BgzfOutStats gst; uint64_t gz_at = 0, tcarry = 0;                  // bgzf: bytes of the file so far; text in front of `out` that no member holds yet
    // the job is driven by the id file (walk_lines of fileio.h): a turn assembles the records of the whole id lines at hand
    LineWalk w; w.begin = w.end = id_begin; w.piece = env_u64("HARC_AMD_FQOUT_PIECE", (uint64_t)256 << 20); w.geom = gq[0];
    uint64_t r0 = 0, out_at = 0; int npieces = 0; bool over = false;
    if (!(stop_at_nrec && nrec == 0)) RC_TRY(walk_lines(c, in.id_path, isz, &w, [&](CarriedText &ids, LineTurn &t) -> int {
        if (stop_at_nrec && r0 + t.whole >= nrec) RC_TRY(ids.end_at(&t, nrec - r0));         // the lines of this output end in the piece: what follows belongs to the next output
        const uint64_t m = t.whole;
        if (r0 + m > nrec) over = true;                                                      // more ids than reads: the lines are still counted, for the message
        if (over) return HARC_AMD_OK;
        const uint64_t nb = m * LL, out_bytes = fq_text_bytes(third, t.cut + ((t.open && m == t.lines) ? 1 : 0), m, L);      // (a last line of the FILE without its newline is one)
        RC_TRY(dev_reserve(&dna, (size_t)nb)); RC_TRY(dev_reserve(&qual, (size_t)nb)); RC_TRY(dev_reserve(&out, (size_t)(tcarry + out_bytes), (size_t)tcarry));
        // lines [rec_base + r0, rec_base + r0 + m) of the two fixed-width files, by offset
        const uint64_t f0 = (rec_base + r0) * LL, f1 = (rec_base + r0 + m) * LL;
        FileFeeder fd(c, in.dna_path), fq(c, in.quality_path);                               // (the feeders wait for the stream when they go)
        RC_TRY(fd.start({ { f0, f1 } }, gq[1])); RC_TRY(fq.start({ { f0, f1 } }, gq[2]));
        const double t0 = mono_now();
        RC_TRY(fd.upload_piece(0, dna.p, nullptr)); RC_TRY(fq.upload_piece(0, qual.p, nullptr));
        t_read += mono_now() - t0;
        RC_TRY(timer.begin(c->stream));
        RC_TRY(harc_idmate_apply_lines(c, t.text, t.nls, m, rule, d_bad));                   // (nothing for the rules that patch nothing)
        RC_TRY(fq_run(c, t.text, t.nls, dna.p, qual.p, (uint32_t)m, L, out.p + tcarry, out_bytes, d_err, third));
        RC_TRY(timer.end_mark(c->stream));
        if (!bgzf) { const double t0w = mono_now(); RC_TRY(drain.put(out.p, (size_t)out_bytes, out_at)); t_write += mono_now() - t0w; }
        else {
            const uint64_t have = tcarry + out_bytes, full = have / DM_TEXT * DM_TEXT;
            if (full) {
                uint64_t ngz = 0;
                RC_TRY(dev_reserve(&gz, (size_t)dm_bound(full)));
                RC_TRY(harc_bgzf_deflate(c, out.p, full, 0, (uint8_t *)gz.p, gz.cap, &ngz, &gst));
                { const double t0w = mono_now(); RC_TRY(drain.put(gz.p, (size_t)ngz, gz_at)); t_write += mono_now() - t0w; }
                gz_at += ngz;
                if (have > full) HIP_TRY(hipMemcpyAsync(out.p, out.p + full, (size_t)(have - full), hipMemcpyDeviceToDevice, c->stream));     // (less than a member: no overlap)
            }
            tcarry = have - full;
        }
        out_at += out_bytes; npieces++; r0 += m;
        return timer.end_wait();
    }));
    *id_end = w.end; t_read += w.t_read;
    if (over || r0 != nrec) { on_mismatch(w.lines); return HARC_AMD_EINVAL; }
    if (!stop_at_nrec && out_at != out_size) { harc_set_error("fastq_assemble_files: %llu bytes assembled, the file sizes announce %llu", (unsigned long long)out_at, (unsigned long long)out_size); return HARC_AMD_EINTERNAL; }
    RC_TRY(fq_check_errors(c, d_err, L));
    {
        unsigned long long bad = 0;
        HIP_TRY(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (bad) {
            harc_set_error("fastq_assemble_pair_files: %llu id lines of %s do not carry the '1' that the mate rule '%s' turns into '2': the id file is damaged or another rule was recorded than the one that holds",
                           bad, in.id_path, idm_rule_name(rule));
            return HARC_AMD_EINVAL;
        }
    }
    if (bgzf) {                                                       // the last member and the end-of-file marker
        uint64_t ngz = 0;
        RC_TRY(dev_reserve(&gz, (size_t)dm_bound(tcarry)));
        RC_TRY(harc_bgzf_deflate(c, out.p, tcarry, 1, (uint8_t *)gz.p, gz.cap, &ngz, &gst));
        { const double t0w = mono_now(); RC_TRY(drain.put(gz.p, (size_t)ngz, gz_at)); t_write += mono_now() - t0w; }
        gz_at += ngz;
        drain.set_final_size(gz_at);
    } else if (stop_at_nrec) drain.set_final_size(out_at);
    { const double t0 = mono_now(); RC_TRY(drain.finish()); t_write += mono_now() - t0; }
    if (tlog && bgzf) fprintf(stderr, "[fastq_out] %llu bytes in %d pieces: %.3f s in the kernel, %.3f s waiting for the readers, %.3f s waiting for the writers; BGZF: %llu bytes of text -> %llu bytes in %llu members (%llu stored), %.3f s in the deflate kernels\n",
                              (unsigned long long)out_at, npieces, t_kernel, t_read, t_write, (unsigned long long)gst.text, (unsigned long long)gz_at, (unsigned long long)gst.members,
                              (unsigned long long)gst.stored, gst.seconds);
    else if (tlog) fprintf(stderr, "[fastq_out] %llu bytes in %d pieces: %.3f s in the kernel, %.3f s waiting for the readers, %.3f s waiting for the writers\n",
                      (unsigned long long)out_at, npieces, t_kernel, t_read, t_write);
    return HARC_AMD_OK;
}

extern "C" int harc_amd_fastq_assemble_files_ex(const harc_amd_params *params, const char *dna_path, const char *id_path, const char *quality_path, const char *out_path,
                                                int32_t bgzf)
{
    return harc_amd_fastq_assemble_third_files(params, dna_path, id_path, quality_path, out_path, bgzf, TH_BARE);
}
// third (third.h): TH_SAME writes '+' and id[1..] as the third line of every record, anything else a bare '+'
extern "C" int harc_amd_fastq_assemble_third_files(const harc_amd_params *params, const char *dna_path, const char *id_path, const char *quality_path, const char *out_path,
                                                   int32_t bgzf, int32_t third)
{
    RC_TRY(fq_check_third("fastq_assemble_files", third));
    if (!params || !dna_path || !id_path || !quality_path || !out_path) { harc_set_error("fastq_assemble_files: bad arguments"); return HARC_AMD_EINVAL; }
    FqInputs in;
    RC_TRY(fq_probe("fastq_assemble_files", dna_path, id_path, quality_path, &in));
    CtxGuard guard;
    RC_TRY(side_context(params, in.L, &guard.c));
    harc_amd_ctx *c = guard.c;
    // the ring is split into four quarters of four slices each and reserved whole before any mover starts.  With the default slice of 64 MB that is the 1 GiB the
    // ring always had.  HARC_AMD_FEED_SLICE sets the slice, HARC_AMD_FEED_THREADS the host threads of all four together.
    RingGeom gq[4];
    RC_TRY(ring_split(c, 4, 4, "FASTQ output", gq));
    OutFileGuard outguard{ out_path };
    uint64_t id_end = 0;
    RC_TRY(fq_assemble_part(c, gq, in, 0, 0, in.n, false, IDM_NONE, third, out_path, bgzf, &id_end, [&](uint64_t seen) {
        harc_set_error("fastq_assemble_files: %s holds %llu lines, %s %llu reads", id_path, (unsigned long long)seen, dna_path, (unsigned long long)in.n);
    }));
    outguard.ok = true;
    return HARC_AMD_OK;
}

// The two FASTQ files of a paired archive (./harc -d -p -q): the reads and quality values of file 1 are records [0, n), those of file 2 records [n, 2 n) of the
// fixed-stride files.  rule none: the id file holds 2 n lines, file 2 continues where file 1 stopped.  Any other rule: it holds file 1's n lines, and file 2's
// are made from them on the GPU, a piece at a time, in front of the tile kernel.  On any failure neither output file is left.
extern "C" int harc_amd_fastq_assemble_pair_files(const harc_amd_params *params, const char *dna_path, const char *id_path, const char *quality_path, const char *out1_path,
                                                  const char *out2_path, uint64_t records_per_file, int32_t rule, int32_t bgzf)
{
    return harc_amd_fastq_assemble_third_pair_files(params, dna_path, id_path, quality_path, out1_path, out2_path, records_per_file, rule, bgzf, TH_BARE);
}
// ... under the rule same of the third lines, file 2's third lines carry file 2's ids: the patch kernel runs in front of the assembly
extern "C" int harc_amd_fastq_assemble_third_pair_files(const harc_amd_params *params, const char *dna_path, const char *id_path, const char *quality_path, const char *out1_path,
                                                        const char *out2_path, uint64_t records_per_file, int32_t rule, int32_t bgzf, int32_t third)
{
    RC_TRY(fq_check_third("fastq_assemble_pair_files", third));
    if (!params || !dna_path || !id_path || !quality_path || !out1_path || !out2_path) { harc_set_error("fastq_assemble_pair_files: bad arguments"); return HARC_AMD_EINVAL; }
    if (rule < IDM_NONE || rule > IDM_SPACE) { harc_set_error("fastq_assemble_pair_files: %d is no mate rule (0 none, 1 same, 2 slash, 3 space)", (int)rule); return HARC_AMD_EINVAL; }
    FqInputs in;
    RC_TRY(fq_probe("fastq_assemble_pair_files", dna_path, id_path, quality_path, &in));
    const uint64_t n = records_per_file;
    if (in.n != 2 * n) {
        harc_set_error("fastq_assemble_pair_files: %s holds %llu reads, the pair record announces 2 x %llu", dna_path, (unsigned long long)in.n, (unsigned long long)n);
        return HARC_AMD_EINVAL;
    }
    CtxGuard guard;
    RC_TRY(side_context(params, in.L, &guard.c));
    harc_amd_ctx *c = guard.c;
    RingGeom gq[4];
    RC_TRY(ring_split(c, 4, 4, "FASTQ output", gq));
    OutFileGuard guard1{ out1_path }, guard2{ out2_path };
    const uint64_t want = rule == IDM_NONE ? 2 * n : n;
    uint64_t id_end = 0, taken = 0;
    auto refuse = [&](uint64_t seen) {
        harc_set_error("fastq_assemble_pair_files: %s holds %s%llu lines, %llu are needed (%llu records in each file, ids %s)", id_path, (rule == IDM_NONE && !taken) ? "only " : "",
                       (unsigned long long)(taken + seen), (unsigned long long)want, (unsigned long long)n, idm_rule_name(rule));
    };
    if (rule == IDM_NONE) {
        RC_TRY(fq_assemble_part(c, gq, in, 0, 0, n, true, IDM_NONE, third, out1_path, bgzf, &id_end, refuse));
        taken = n;
        const uint64_t from = id_end;
        RC_TRY(fq_assemble_part(c, gq, in, from, n, n, false, IDM_NONE, third, out2_path, bgzf, &id_end, refuse));
    } else {
        RC_TRY(fq_assemble_part(c, gq, in, 0, 0, n, false, IDM_SAME, third, out1_path, bgzf, &id_end, refuse));
        RC_TRY(fq_assemble_part(c, gq, in, 0, n, n, false, rule, third, out2_path, bgzf, &id_end, refuse));
    }
    guard1.ok = guard2.ok = true;
    return HARC_AMD_OK;
}
