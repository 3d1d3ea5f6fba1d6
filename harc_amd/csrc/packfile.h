// packfile.h -- the way back to text that the packed side files share (qpack.hip: X.quality.hq, idpack.hip: X.id.hi).  Such a file is a 32-byte header and then
// self-delimiting blocks: a prefix says how many bytes a block holds, and a kernel with a workgroup per block turns the blocks into one contiguous text.  Here, once:
// the walk over the prefixes on the host, the run of the decode kernel with its error word, the device call and the file call.  A format hands in a PackFormat.
#pragma once
#include "fileio.h"

#define PF_HEADER 32u
struct PackHeader { uint32_t L = 0, rb = 0; uint64_t n = 0, nb = 0, text = 0; };      // lines of L (0: of any length) in blocks of rb: n lines, nb blocks, `text` bytes of text
static inline uint32_t pack_block_lines(const PackHeader &H, uint64_t b) { const uint64_t line0 = b * (uint64_t)H.rb; return H.n - line0 < H.rb ? (uint32_t)(H.n - line0) : H.rb; }

struct PackFormat {
    const char *tag;                                              // "q" / "id": <tag>unpack... in the messages, [<tag>pack] in the trace
    const char *ring;                                             // "quality" / "id": whose pinned ring it is, in the messages
    const char *piece_env; uint64_t piece_default;                // the file call: blocks a piece
    uint32_t prefix_bytes;                                        // what the prefix rule reads, at most 16
    int (*parse_header)(const char *who, const uint8_t *h, uint64_t n_bytes, PackHeader *H);
    // the format's prefix rule for block b: q and `left` as qv_prefix / id_prefix take them -> 1 with the bytes of its payload and of its text, or 0
    int (*prefix)(const PackHeader &H, uint64_t b, const uint8_t *q, uint64_t left, uint64_t text_left, uint64_t *payload_bytes, uint64_t *text_bytes);
    // the one-lane walk kernel over a packed form in device memory: off / toff[0 .. nb] relative to the first block, bad[0]: 1 + the first block that the prefix rule
    // refuses (nb + 1: bytes are left behind the last block, nb + 2: the text bytes of the blocks are not those of the header), bad[1]: its byte
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
