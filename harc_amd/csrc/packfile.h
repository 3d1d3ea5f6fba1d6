// packfile.h -- what the packed side files share (qpack.hip: X.quality.hq, idpack.hip: X.id.hi, spack.hip: X.hs).  Such a file is a 32-byte header and then
// self-delimiting blocks: a prefix says how many bytes a block holds, and a kernel with a workgroup per block turns text into blocks or blocks into one contiguous text.
// The way in, once: the coded branch of the gather kernels (pack_gather_coded), the run of encode, scan and gather with its error words and its capacity refusal
// (pack_run) and the device call (pack_device); a format hands in its scratch, its launches and its messages as hooks.  The way back, once: the walk over the
// prefixes on the host (pack_walk) and in one lane of the device (k_pack_walk), the run of the decode kernel with its error word, the host call, the device call
// and the file call.  A format hands in a PackFormat.
#pragma once
#include "devutil.h"
#include "qv_block.h"
#include "fileio.h"

#define PF_HEADER 32u
struct PackHeader { uint32_t L = 0, rb = 0; uint64_t n = 0, nb = 0, text = 0; };      // lines of L (0: of any length) in blocks of rb: n lines, nb blocks, `text` bytes of text
QV_HD uint32_t pack_block_lines(const PackHeader &H, uint64_t b) { const uint64_t line0 = b * (uint64_t)H.rb; return H.n - line0 < H.rb ? (uint32_t)(H.n - line0) : H.rb; }

struct PackFormat {
    const char *tag;                                              // "q" / "id": <tag>unpack... in the messages, [<tag>pack] in the trace
    const char *ring;                                             // "quality" / "id": whose pinned ring it is, in the messages
    const char *piece_env; uint64_t piece_default;                // the file call: blocks a piece
    uint32_t prefix_bytes;                                        // what the prefix rule reads, at most 16
    int (*parse_header)(const char *who, const uint8_t *h, uint64_t n_bytes, PackHeader *H);
    // the format's prefix rule for block b: q and `left` as qv_prefix / id_prefix take them -> 1 with the bytes of its payload and of its text, or 0
    int (*prefix)(const PackHeader &H, uint64_t b, const uint8_t *q, uint64_t left, uint64_t text_left, uint64_t *payload_bytes, uint64_t *text_bytes);
    // the one-lane walk kernel over a packed form in device memory, pack_walk_device<Rule> with the rule above: off / toff[0 .. nb] relative to the first block,
    // bad[0]: 1 + the first block that the prefix rule refuses (nb + 1: bytes are left behind the last block, nb + 2: the text bytes of the blocks are not those of
    // the header), bad[1]: its byte
    void (*walk)(harc_amd_ctx *c, const uint8_t *d_packed, uint64_t n_bytes, const PackHeader &H, uint64_t *d_off, uint64_t *d_toff, unsigned long long *d_bad);
    // the decode kernel over nb blocks with n lines: it lowers *d_errw to block << 8 | code for a block that is damaged
    void (*decode)(harc_amd_ctx *c, const uint8_t *d_blocks, const uint64_t *d_off, const uint64_t *d_toff, uint32_t nb, uint64_t n, const PackHeader &H, char *d_text, unsigned long long *d_errw);
    const char *(*error_text)(uint32_t code);
};

// the refusals of a walk.  `what`: "the packed form" or the file's name
static inline int pack_refuse_prefix(const char *who, const char *what, const PackHeader &H, uint64_t n_bytes, uint64_t b, uint64_t at)
{
    harc_set_error("%s: block %llu at byte %llu leaves the %llu bytes of %s or the %llu bytes of its text", who, (unsigned long long)b, (unsigned long long)at, (unsigned long long)n_bytes, what, (unsigned long long)H.text);
    return HARC_AMD_EINVAL;
}
static inline int pack_check_ends(const char *who, const char *what, const PackHeader &H, uint64_t n_bytes, uint64_t at, uint64_t tat)
{
    if (at != n_bytes) { harc_set_error("%s: block %llu ends at byte %llu, but %s holds %llu bytes", who, (unsigned long long)H.nb - 1, (unsigned long long)at, what, (unsigned long long)n_bytes); return HARC_AMD_EINVAL; }
    if (tat != H.text) { harc_set_error("%s: block %llu ends the text at byte %llu, the header of %s announces %llu", who, (unsigned long long)H.nb - 1, (unsigned long long)tat, what, (unsigned long long)H.text); return HARC_AMD_EINVAL; }
    return HARC_AMD_OK;
}
static inline int pack_refuse_damaged(const PackFormat &F, uint64_t b, uint64_t at, uint32_t code)
{
    harc_set_error("%sunpack: block %llu at byte %llu is damaged: %s", F.tag, (unsigned long long)b, (unsigned long long)at, F.error_text(code));
    return HARC_AMD_EINVAL;
}

// The walk over the prefixes of the H.nb blocks of a packed form of n_bytes bytes.  read(at, q, k) fetches the k <= F.prefix_bytes bytes at byte `at`; block(b, at,
// payload_bytes, tat) sees every block as soon as its prefix has passed and before the prefix of the next is looked at.  off / toff[0 .. nb] (both or neither): where
// the blocks and their texts start and, [nb], end.  Refused: a block that leaves the bytes or the text, bytes behind the last block, text bytes that are not the header's.
// upto < H.nb: the walk ends behind block upto - 1 (a range restore: what lies behind the blocks it needs is neither read nor checked), off / toff[0 .. upto]
template <class Read, class Block>
static int pack_walk(const PackFormat &F, const char *who, const char *what, const PackHeader &H, uint64_t n_bytes, Read read, Block block, uint64_t *off, uint64_t *toff, uint64_t upto = ~0ull)
{
    uint64_t at = PF_HEADER, tat = 0;
    const uint64_t nb = upto < H.nb ? upto : H.nb;
    for (uint64_t b = 0; b < nb; b++) {
        if (off) { off[b] = at; toff[b] = tat; }
        uint8_t q[16]; uint64_t pb = 0, tb = 0;
        const uint64_t left = n_bytes - at;
        RC_TRY(read(at, q, (size_t)(left < F.prefix_bytes ? left : F.prefix_bytes)));
        if (!F.prefix(H, b, q, left, H.text - tat, &pb, &tb)) return pack_refuse_prefix(who, what, H, n_bytes, b, at);
        RC_TRY(block(b, at, pb, tat));
        at += 4 + pb; tat += tb;
    }
    if (off) { off[nb] = at; toff[nb] = tat; }
    return nb == H.nb ? pack_check_ends(who, what, H, n_bytes, at, tat) : HARC_AMD_OK;
}

// The same walk by one lane over a packed form in device memory, what PackFormat::walk launches.  Rule::prefix is the format's prefix rule, PackFormat::prefix as
// a __host__ __device__ function.  off and toff are filled for every format, also where the text of a block follows from its number alone, and both ends are
// checked for every format: the drivers above allocate and read both
template <class Rule>
__global__ void k_pack_walk(const uint8_t *p, uint64_t n_bytes, PackHeader H, uint64_t *off, uint64_t *toff, unsigned long long *bad)
{
    if (threadIdx.x || blockIdx.x) return;
    uint64_t at = PF_HEADER, tat = 0;
    for (uint64_t b = 0; b < H.nb; b++) {
        off[b] = at - PF_HEADER; toff[b] = tat;
        uint64_t pb = 0, tb = 0;
        if (!Rule::prefix(H, b, p + at, n_bytes - at, H.text - tat, &pb, &tb)) { bad[0] = b + 1; bad[1] = at; return; }
        at += 4 + pb; tat += tb;
    }
    off[H.nb] = at - PF_HEADER; toff[H.nb] = tat;
    if (at != n_bytes || tat != H.text) { bad[0] = H.nb + (at != n_bytes ? 1 : 2); bad[1] = at != n_bytes ? at : tat; }
}
template <class Rule>
static void pack_walk_device(harc_amd_ctx *c, const uint8_t *d_packed, uint64_t n_bytes, const PackHeader &H, uint64_t *d_off, uint64_t *d_toff, unsigned long long *d_bad)
{
    hipLaunchKernelGGL(k_pack_walk<Rule>, dim3(1), dim3(64), 0, c->stream, d_packed, n_bytes, H, d_off, d_toff, d_bad);
}

// harc_amd_<tag>unpack_host: a packed form in host memory -> its text, block after block.  text == nullptr: the size alone.  decode(H, payload, payload_bytes,
// lines, text) is the host's block rule: 0, or the format's code of what is damaged
template <class Decode>
static int pack_unpack_host(const PackFormat &F, const uint8_t *packed, uint64_t n_bytes, uint8_t *text, uint64_t cap, uint64_t *n_out, Decode decode)
{
    char who[32]; snprintf(who, sizeof who, "%sunpack_host", F.tag);
    if (!packed || !n_out) { harc_set_error("%s: bad arguments", who); return HARC_AMD_EINVAL; }
    if (n_bytes < PF_HEADER) { harc_set_error("%s: %llu bytes are fewer than the %u of the header", who, (unsigned long long)n_bytes, PF_HEADER); return HARC_AMD_EINVAL; }
    PackHeader H;
    RC_TRY(F.parse_header(who, packed, n_bytes, &H));
    *n_out = H.text;
    if (!text) return HARC_AMD_OK;
    if (cap < H.text) { harc_set_error("%s: the text takes %llu bytes, the buffer holds %llu", who, (unsigned long long)H.text, (unsigned long long)cap); return HARC_AMD_EINVAL; }
    return pack_walk(F, who, "the packed form", H, n_bytes,
                     [&](uint64_t at, uint8_t *q, size_t k) { memcpy(q, packed + at, k); return HARC_AMD_OK; },
                     [&](uint64_t b, uint64_t at, uint64_t pb, uint64_t tat) {
                         const int e = decode(H, packed + at + 4, (uint32_t)pb, pack_block_lines(H, b), text + tat);
                         return e ? pack_refuse_damaged(F, b, at, (uint32_t)e) : HARC_AMD_OK;
                     }, nullptr, nullptr);
}

// nb blocks at d_blocks with their offsets d_off[0 .. nb] and text offsets d_toff[0 .. nb] -> the n lines at d_text.  block0 / base: number and file offset of the
// first of them, h_off: d_off on the host, for the message
static int pack_unpack_run(harc_amd_ctx *c, const PackFormat &F, const PackHeader &H, const uint8_t *d_blocks, const uint64_t *d_off, const uint64_t *d_toff, const uint64_t *h_off,
                           uint32_t nb, uint64_t n, char *d_text, uint64_t block0, uint64_t base)
{
    if (!nb) return HARC_AMD_OK;
    PoolScope scope(c);
    unsigned long long *d_errw = nullptr; RC_TRY(dalloc(c, &d_errw, 2));
    HIP_TRY(hipMemsetAsync(d_errw, 0xFF, 8, c->stream));
    F.decode(c, d_blocks, d_off, d_toff, nb, n, H, d_text, d_errw);
    HIP_TRY(hipGetLastError());
    unsigned long long errw = 0;
    HIP_TRY(hipMemcpyAsync(&errw, d_errw, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (errw != ~0ull) { const uint64_t b = errw >> 8; return pack_refuse_damaged(F, block0 + b, base + (h_off ? h_off[b] : 0), (uint32_t)(errw & 0xFF)); }
    return HARC_AMD_OK;
}

// harc_amd_<tag>unpack_device: a packed form in device memory -> its text.  d_text == nullptr: the size alone
static int pack_unpack_device(const PackFormat &F, harc_amd_ctx *c, const uint8_t *d_packed, uint64_t n_bytes, char *d_text, uint64_t out_capacity, uint64_t *n_out)
{
    char who[32]; snprintf(who, sizeof who, "%sunpack_device", F.tag);
    if (!c || !d_packed || !n_out) { harc_set_error("%s: bad arguments", who); return HARC_AMD_EINVAL; }
    if (n_bytes < PF_HEADER) { harc_set_error("%s: %llu bytes are fewer than the %u of the header", who, (unsigned long long)n_bytes, PF_HEADER); return HARC_AMD_EINVAL; }
    HIP_TRY(hipSetDevice(c->P.device));
    uint8_t h[PF_HEADER];
    HIP_TRY(hipMemcpyAsync(h, d_packed, PF_HEADER, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    PackHeader H;
    RC_TRY(F.parse_header(who, h, n_bytes, &H));
    *n_out = H.text;
    if (!d_text) return HARC_AMD_OK;
    if (out_capacity < H.text) { harc_set_error("%s: the text takes %llu bytes, the buffer holds %llu", who, (unsigned long long)H.text, (unsigned long long)out_capacity); return HARC_AMD_EINVAL; }
    if (!H.nb) return HARC_AMD_OK;
    if (H.nb > 0x7FFFFFF0ull) { harc_set_error("%s: too many blocks for one call", who); return HARC_AMD_EINVAL; }
    PoolScope scope(c);
    uint64_t *d_off = nullptr, *d_toff = nullptr; unsigned long long *d_bad = nullptr;
    RC_TRY(dalloc(c, &d_off, (size_t)H.nb + 1)); RC_TRY(dalloc(c, &d_toff, (size_t)H.nb + 1)); RC_TRY(dalloc(c, &d_bad, 2));
    HIP_TRY(hipMemsetAsync(d_bad, 0, 16, c->stream));
    F.walk(c, d_packed, n_bytes, H, d_off, d_toff, d_bad);
    HIP_TRY(hipGetLastError());
    unsigned long long bad[2] = { 0, 0 };
    std::vector<uint64_t> h_off((size_t)H.nb + 1);
    HIP_TRY(hipMemcpyAsync(bad, d_bad, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (bad[0] == H.nb + 2) return pack_check_ends(who, "the packed form", H, n_bytes, n_bytes, bad[1]);
    if (bad[0] == H.nb + 1) return pack_check_ends(who, "the packed form", H, n_bytes, bad[1], H.text);
    if (bad[0]) return pack_refuse_prefix(who, "the packed form", H, n_bytes, bad[0] - 1, bad[1]);
    HIP_TRY(hipMemcpyAsync(h_off.data(), d_off, 8 * ((size_t)H.nb + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return pack_unpack_run(c, F, H, d_packed + PF_HEADER, d_off, d_toff, h_off.data(), (uint32_t)H.nb, H.n, d_text, 0, PF_HEADER);
}

// harc_amd_<tag>unpack_files: the packed file goes through the feeder's half of the ring in pieces of whole blocks, its text through the drain's.
// shared: a side context of the caller's that serves several files one after the other, slice: its slice of the ring (spack.hip); nullptr, 0: the call's own, the default
// range (may be null: the whole file): lines [range[0], range[0] + range[1]) alone are written.  The prefixes are walked up to the last block that holds one of
// them, the blocks from the first such block on go to the decoder, and the text of the first and the last is cut in device memory: by the stride where the header
// names a line length, else where the line select kernel (linesel.hip) finds the line.  Blocks outside the range are neither read nor checked
static int pack_unpack_files(const PackFormat &F, const harc_amd_params *params, const char *packed_path, const char *out_path, harc_amd_ctx *shared = nullptr, size_t slice = 0,
                             const uint64_t *range = nullptr)
{
    char who[32]; snprintf(who, sizeof who, range ? "%sunpack_range_files" : "%sunpack_files", F.tag);
    if (!params || !packed_path || !out_path) { harc_set_error("%s: bad arguments", who); return HARC_AMD_EINVAL; }
    uint64_t fsz = 0;
    if (!file_size(packed_path, &fsz)) { harc_set_error("cannot open %s", packed_path); return HARC_AMD_EIO; }
    OutFileGuard outguard{ out_path };
    if (fsz < PF_HEADER) { harc_set_error("%s: %s holds %llu bytes, fewer than the %u of the header", who, packed_path, (unsigned long long)fsz, PF_HEADER); return HARC_AMD_EINVAL; }
    const int fd = open(packed_path, O_RDONLY);
    if (fd < 0) { harc_set_error("cannot open %s", packed_path); return HARC_AMD_EIO; }
    struct FdGuard { int fd; ~FdGuard() { close(fd); } } fdguard{ fd };
    uint64_t bytes_read = 0;                                      // by the walk; the blocks that go to the decoder are added below
    auto read = [&](uint64_t at, uint8_t *q, size_t k) { bytes_read += k; if (pread(fd, q, k, (off_t)at) == (ssize_t)k) return HARC_AMD_OK; harc_set_error("cannot read %s", packed_path); return HARC_AMD_EIO; };
    uint8_t h[PF_HEADER];
    RC_TRY(read(0, h, PF_HEADER));
    PackHeader H;
    RC_TRY(F.parse_header(who, h, fsz, &H));
    uint64_t blk0 = 0, blk1 = H.nb;                               // the blocks [blk0, blk1) are decoded
    if (range) {
        if (range[1] == 0 || range[0] >= H.n || range[1] > H.n - range[0]) {
            harc_set_error("%s: lines %llu .. %llu are wanted, %s holds %llu lines", who, (unsigned long long)range[0] + 1, (unsigned long long)(range[0] + range[1]), packed_path, (unsigned long long)H.n);
            return HARC_AMD_EINVAL;
        }
        blk0 = range[0] / H.rb; blk1 = (range[0] + range[1] - 1) / H.rb + 1;
    }
    // the block offsets and the places in the text, from the prefixes: known, and inside the file, before a device is touched
    std::vector<uint64_t> off((size_t)blk1 + 1), toff((size_t)blk1 + 1);
    RC_TRY(pack_walk(F, who, packed_path, H, fsz, read, [](uint64_t, uint64_t, uint64_t, uint64_t) { return HARC_AMD_OK; }, off.data(), toff.data(), blk1));
    bytes_read += off[blk1] - off[blk0];
    CtxGuard guard;
    if (!shared) RC_TRY(side_context(params, H.L ? (int)H.L : 100, &guard.c));
    harc_amd_ctx *c = shared ? shared : guard.c;
    RingGeom g[2];                                                // the feeder's and the drain's
    RC_TRY(ring_split(c, 2, 8, F.ring, g, slice));
    DevBuf pk{ c }, txt{ c }, doff{ c };
    const bool tlog = getenv("HARC_AMD_TRACE") != nullptr;
    double t_read = 0, t_write = 0, t_kernel = 0;
    const uint64_t piece_blocks = env_u64(F.piece_env, F.piece_default);
    int npieces = 0; uint64_t out_at = 0;
    {
        FileDrain drain(c);
        RC_TRY(drain.start(out_path, (size_t)(toff[blk1] - toff[blk0]), &g[1], true));
        std::vector<std::pair<uint64_t, uint64_t>> pieces;
        for (uint64_t b = blk0; b < blk1; b += piece_blocks) pieces.emplace_back(off[b], off[blk1 - b < piece_blocks ? blk1 : b + piece_blocks]);
        FileFeeder feed(c, packed_path);
        if (!pieces.empty()) RC_TRY(feed.start(pieces, g[0]));
        std::vector<uint64_t> rel;
        for (size_t p = 0; p < pieces.size(); p++) {
            const uint64_t b0 = blk0 + p * piece_blocks, b1 = blk1 - b0 < piece_blocks ? blk1 : b0 + piece_blocks, bytes = pieces[p].second - pieces[p].first, k = b1 - b0 + 1;
            const uint64_t m = (b1 == H.nb ? H.n : b1 * H.rb) - b0 * H.rb, tbytes = toff[b1] - toff[b0];
            RC_TRY(dev_reserve(&pk, (size_t)bytes)); RC_TRY(dev_reserve(&txt, (size_t)tbytes + 1)); RC_TRY(dev_reserve(&doff, 16 * (size_t)k));
            { const double t0 = mono_now(); RC_TRY(feed.upload_piece(p, pk.p, nullptr)); t_read += mono_now() - t0; }
            rel.resize((size_t)(2 * k));
            for (uint64_t b = b0; b <= b1; b++) { rel[(size_t)(b - b0)] = off[b] - off[b0]; rel[(size_t)(k + b - b0)] = toff[b] - toff[b0]; }
            HIP_TRY(hipMemcpyAsync(doff.p, rel.data(), 8 * rel.size(), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            { const double t0 = mono_now(); RC_TRY(pack_unpack_run(c, F, H, (const uint8_t *)pk.p, (const uint64_t *)doff.p, (const uint64_t *)doff.p + k, rel.data(), (uint32_t)(b1 - b0), m, txt.p, b0, off[b0])); t_kernel += mono_now() - t0; }
            uint64_t lo = 0, hi = tbytes;                            // what of the piece's text is written
            if (range) {
                // line k of block b, whose text starts `base` bytes into the piece: where it starts in the piece
                auto line_at = [&](uint64_t b, uint64_t kline, uint64_t base, uint64_t *at) -> int {
                    if (H.L) { *at = base + kline * (H.L + 1ull); return HARC_AMD_OK; }
                    uint64_t r[2] = { 0, 0 };
                    RC_TRY(harc_amd_line_offset_device(c, txt.p + base, toff[b + 1] - toff[b], kline, r));
                    if (r[1] == ~0ull) { harc_set_error("%s: the text of block %llu holds %llu lines, line %llu of it is wanted", who, (unsigned long long)b, (unsigned long long)r[0], (unsigned long long)kline); return HARC_AMD_EINVAL; }
                    *at = base + r[1];
                    return HARC_AMD_OK;
                };
                if (b0 == blk0) RC_TRY(line_at(blk0, range[0] - blk0 * H.rb, 0, &lo));
                if (b1 == blk1) RC_TRY(line_at(blk1 - 1, range[0] + range[1] - (blk1 - 1) * H.rb, toff[blk1 - 1] - toff[b0], &hi));
            }
            { const double t0 = mono_now(); RC_TRY(drain.put(txt.p + lo, (size_t)(hi - lo), out_at)); t_write += mono_now() - t0; }
            out_at += hi - lo;
            npieces++;
        }
        drain.set_final_size(out_at);
        { const double t0 = mono_now(); RC_TRY(drain.finish()); t_write += mono_now() - t0; }
    }
    // (a range restore: one status line, with the walk's own count of the bytes it read)
    if (range) printf("[%sunpack] lines %llu .. %llu of %llu: blocks %llu .. %llu of %llu, %llu of the %llu bytes of %s read, %llu bytes of text written\n", F.tag, (unsigned long long)range[0] + 1,
                      (unsigned long long)(range[0] + range[1]), (unsigned long long)H.n, (unsigned long long)blk0, (unsigned long long)blk1 - 1, (unsigned long long)H.nb, (unsigned long long)bytes_read,
                      (unsigned long long)fsz, packed_path, (unsigned long long)out_at);
    if (tlog) fprintf(stderr, "[%spack] unpacked %llu bytes of text from %llu bytes in %llu blocks, %d pieces: %.3f s in the kernels, %.3f s waiting for the readers, %.3f s waiting for the writers\n",
                      F.tag, (unsigned long long)H.text, (unsigned long long)fsz, (unsigned long long)H.nb, npieces, t_kernel, t_read, t_write);
    outguard.ok = true;
    return HARC_AMD_OK;
}

// ------------------------------------------------------------------------------------------------ the way in: text -> blocks
// A format's encode kernel (a workgroup of PF_T per block, lane t owns strand t) codes every block into scratch: a head that holds the PF_T u32 strand lengths
// somewhere, and the strands.  It leaves the block's size with its u32 prefix in bsize[b], its mode (0: stored) in bmode[b] and what went wrong in err[0 .. 3].
#define PF_T 256
struct PackGather { uint32_t scan[PF_T / 64 + 1], soff[PF_T], slen[PF_T]; };                // the LDS of a gather kernel
struct PackStats { uint64_t text = 0, bytes = 0, blocks = 0, mode[3] = { 0, 0, 0 }; double seconds = 0; };      // mode[0]: stored blocks
struct PackBlocks { uint32_t nb; uint32_t *bsize, *bmode; uint64_t *boff; unsigned int *err; };                 // what pack_run allocates for every format

// The coded branch of a gather kernel, behind the u32 prefix that the kernel has written at dst: the head at hdr, whose strand lengths start at lens, and the
// strands go to their byte-granular place behind dst + 4 -- whole dwords of the destination, the bytes in front of and behind them one by one, a wave per
// strand.  payload: the bytes of head and strands together, so that the head is what the strands leave of it.  strand(s, n): where the n > 0 bytes of strand s lie
template <class Strand>
__device__ __forceinline__ void pack_gather_coded(PackGather &S, uint8_t *dst, uint32_t payload, const uint8_t *hdr, const uint8_t *lens, Strand strand)
{
    const uint32_t t = threadIdx.x;
    const uint32_t len = qv_le32(lens + 4u * t);
    uint32_t total;
    const uint32_t off = block_excl_scan_u32<PF_T>(len, S.scan, &total);
    const uint32_t h = payload - total;
    S.soff[t] = off; S.slen[t] = len;
    group_copy_bytes(dst + 4, hdr, h, t, PF_T);
    __syncthreads();
    const uint32_t wv = t >> 6, lane = t & 63u;
    for (uint32_t s = wv; s < PF_T; s += PF_T / 64) {
        const uint32_t n = S.slen[s];
        if (n) group_copy_bytes(dst + 4 + h + S.soff[s], strand(s, n), n, lane, 64);
    }
}

// The blocks alone (no file header) of nb64 <= max_blocks blocks of text_bytes bytes of text -> d_out[0 .. *n_out); d_out == nullptr: the size alone.  Sizes are
// needed before bytes can be placed: encode into scratch, scan the sizes, gather.  tag: "qpack" / "idpack" / "spack" in the messages.  The hooks of the format:
//   scratch(B)    allocates its own scratch from the pool (this function brackets it) and presets err where 0 is not its neutral value
//   encode(B)     launches its encode kernel
//   errors(e, st) reads the four error words: a refusal with its message, or OK with the blocks of each mode added to st->mode (st may be null)
//   gather(B, o)  launches its gather kernel to o
template <class Scratch, class Encode, class Errors, class Gather>
static int pack_run(harc_amd_ctx *c, const char *tag, uint64_t nb64, uint64_t max_blocks, uint64_t text_bytes, uint8_t *d_out, uint64_t out_capacity, uint64_t *n_out, PackStats *st,
                    Scratch scratch, Encode encode, Errors errors, Gather gather)
{
    *n_out = 0;
    if (nb64 > max_blocks) { harc_set_error("%s: too many blocks for one call", tag); return HARC_AMD_EINVAL; }
    PackBlocks B = { (uint32_t)nb64, nullptr, nullptr, nullptr, nullptr };
    const size_t nb = B.nb;
    if (!nb) return HARC_AMD_OK;
    PoolScope scope(c);
    RC_TRY(dalloc(c, &B.bsize, nb + 1)); RC_TRY(dalloc(c, &B.bmode, nb)); RC_TRY(dalloc(c, &B.boff, nb + 1)); RC_TRY(dalloc(c, &B.err, 4));
    HIP_TRY(hipMemsetAsync(B.bsize + nb, 0, 4, c->stream));
    HIP_TRY(hipMemsetAsync(B.err, 0, 16, c->stream));
    RC_TRY(scratch(B));
    KernelTimer timer(st ? &st->seconds : nullptr);
    RC_TRY(timer.begin(c->stream));
    encode(B);
    HIP_TRY(hipGetLastError());
    RC_TRY(prim_excl_scan_u32_to_u64(c, B.bsize, B.boff, nb + 1));
    uint64_t total = 0; unsigned int err[4] = { 0, 0, 0, 0 };
    HIP_TRY(hipMemcpyAsync(&total, B.boff + nb, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(err, B.err, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    RC_TRY(errors(err, st));
    *n_out = total;
    if (st) { st->text += text_bytes; st->bytes += total; st->blocks += nb; }
    if (d_out) {
        // the size first: a buffer that is too small is refused with both numbers before a byte of it is written
        if (out_capacity < total) { harc_set_error("%s_device: the blocks take %llu bytes, the buffer holds %llu", tag, (unsigned long long)total, (unsigned long long)out_capacity); return HARC_AMD_EINVAL; }
        gather(B, d_out);
        HIP_TRY(hipGetLastError());
    }
    RC_TRY(timer.end(c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                     // the scratch goes back to the pool
    return HARC_AMD_OK;
}

// harc_amd_<tag>_device: a text in device memory -> its packed form, `head` bytes of file header (0: none) and the blocks.  d_out == nullptr: the size alone.
// args_ok: the format's own argument check.  The hooks of the format:
//   geometry()                 refuses a block geometry that the format cannot hold, with its message
//   run(o, cap, &nblk, st)     its run of pack_run, behind whatever it has to build first (its pool memory inside a scope of its own)
//   header(h)                  the PF_HEADER bytes of the file header, after the run
//   trace(st, n)               its line for HARC_AMD_TRACE, n the bytes of the packed form
template <class Geometry, class Run, class Header, class Trace>
static int pack_device(const char *tag, harc_amd_ctx *c, bool args_ok, uint64_t head, uint8_t *d_out, uint64_t out_capacity, uint64_t *n_out, Geometry geometry, Run run, Header header,
                       Trace trace)
{
    if (!c || !args_ok || !n_out) { harc_set_error("%s_device: bad arguments", tag); return HARC_AMD_EINVAL; }
    RC_TRY(geometry());
    HIP_TRY(hipSetDevice(c->P.device));
    const bool tlog = getenv("HARC_AMD_TRACE") != nullptr;
    PackStats st; uint64_t nblk = 0;
    *n_out = head;
    // the size first: a buffer that is too small is refused with both numbers before a byte of it is written
    if (d_out && out_capacity < head) { harc_set_error("%s_device: the blocks take at least %llu bytes, the buffer holds %llu", tag, (unsigned long long)head, (unsigned long long)out_capacity); return HARC_AMD_EINVAL; }
    const int rc = run(d_out ? d_out + head : nullptr, d_out ? out_capacity - head : 0, &nblk, tlog ? &st : nullptr);
    *n_out = head + nblk;
    if (rc != HARC_AMD_OK) {
        if (d_out && nblk && out_capacity - head < nblk) harc_set_error("%s_device: the packed form takes %llu bytes, the buffer holds %llu", tag, (unsigned long long)(head + nblk), (unsigned long long)out_capacity);
        return rc;
    }
    if (d_out && head) {
        uint8_t h[PF_HEADER];
        header(h);
        HIP_TRY(hipMemcpyAsync(d_out, h, PF_HEADER, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (tlog) trace(st, *n_out);
    return HARC_AMD_OK;
}
