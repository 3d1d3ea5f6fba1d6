// fileio.h -- the two file <-> HBM movers of the library, shared by ingest.hip (FASTQ in), verify.hip (decoded reads out), fastq_out.hip (both at once) and, through
// packfile.h, qpack.hip and idpack.hip: FileFeeder reads a file into device memory, FileDrain writes device memory into a file, each through pinned slices of the
// context's ring (c->feed_ring) worked by a few host threads.  Around them, once each, what every file-level call needs: the probes of a file (size, first line, last
// byte), whole files read and written, the guards of an output file and of a context, the split of the ring and the slice of a short file's ring, the list of pieces
// a file is fed in (bytes, fixed-stride lines), an owning device buffer, a kernel timer, a text whose cut tail is carried on (CarriedText) with the steps of a turn
// over its whole lines (idmate.hip and idpack.hip loop over them their own way), and walk_lines: the one walk over a file of lines of any length (select.hip, fastq_out.hip).
#pragma once
#include "internal.h"
#include <string>
#include <stdlib.h>
#include <time.h>
#include <errno.h>
#include <sys/stat.h>
#include <unistd.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>

// Which part of the context's ONE pinned ring a feeder or a drain works with, and how: `nslices` slices of `slice` bytes from byte `ring_off` of the ring on,
// `nthr` host threads.  The default is what every caller used before the geometry became an argument: the whole ring, 16 slices of 64 MB, 16 threads.
// Two movers alive at the same time must be given disjoint parts (fastq_out.hip splits the ring four ways), and the ring must have been reserved for all of
// them first (harc_ring_reserve): a mover that finds the ring too small replaces it, which is right only when it is alone.
struct RingGeom { size_t slice = (size_t)64 << 20; int nslices = 16; int nthr = 16; size_t ring_off = 0; };
static inline int harc_ring_reserve(harc_amd_ctx *c, size_t bytes, const char *what)
{
    if (c->feed_ring_bytes >= bytes) return HARC_AMD_OK;
    if (c->feed_ring) { (void)hipHostFree(c->feed_ring); c->feed_ring = nullptr; c->feed_ring_bytes = 0; }
    if (hipHostMalloc((void **)&c->feed_ring, bytes) != hipSuccess) { harc_set_error("hipHostMalloc of the %s ring (%zu bytes) failed", what, bytes); return HARC_AMD_ENOMEM; }
    c->feed_ring_bytes = bytes;
    return HARC_AMD_OK;
}
// HARC_AMD_FEED_SLICE / HARC_AMD_FEED_THREADS over a geometry (tests: slices of a few reads)
static inline void harc_ring_geom_env(RingGeom *g)
{
    if (const char *e = getenv("HARC_AMD_FEED_THREADS")) { const int x = atoi(e); if (x >= 1 && x <= 64) g->nthr = x; }
    if (const char *e = getenv("HARC_AMD_FEED_SLICE")) { const long long x = atoll(e); if (x >= 16 && x <= ((long long)1 << 30)) g->slice = (size_t)x; }
}

static inline double mono_now() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
// HARC_AMD_TRACE: "<tag> <what>: <seconds since the last lap> s" on stderr
struct LapTimer {
    const char *tag; bool on = getenv("HARC_AMD_TRACE") != nullptr; double t = mono_now();
    void lap(const char *what) { if (on) { const double n = mono_now(); fprintf(stderr, "%s %s: %.3f s\n", tag, what, n - t); t = n; } }
};

// ------------------------------------------------------------------------------------------------ what the file-level calls share
static inline bool file_size(const char *path, uint64_t *n) { struct stat st; if (stat(path, &st) != 0 || !S_ISREG(st.st_mode)) return false; *n = (uint64_t)st.st_size; return true; }   // regular files only
// the length of the first line of a file that is not empty, for `who`: 1 .. 255
static inline int first_line_length(const char *path, const char *who, uint32_t *L)
{
    char head[257];
    FILE *f = fopen(path, "rb");
    if (!f) { harc_set_error("cannot open %s", path); return HARC_AMD_EIO; }
    const size_t got = fread(head, 1, sizeof head, f);
    fclose(f);
    size_t nl = 0;
    while (nl < got && head[nl] != '\n') nl++;
    if (nl > 255) { harc_set_error("%s: the first line of %s is longer than 255 characters", who, path); return HARC_AMD_EINVAL; }
    if (nl == 0) { harc_set_error("%s: the first line of %s is empty", who, path); return HARC_AMD_EINVAL; }
    *L = (uint32_t)nl;
    return HARC_AMD_OK;
}
// of a file that is not empty
static inline int last_byte_is_newline(const char *path, bool *yes)
{
    FILE *g = fopen(path, "rb"); char last = 0;
    if (!g || fseeko(g, -1, SEEK_END) != 0 || fread(&last, 1, 1, g) != 1) { if (g) fclose(g); harc_set_error("cannot read %s", path); return HARC_AMD_EIO; }
    fclose(g);
    *yes = last == '\n';
    return HARC_AMD_OK;
}
// A whole file into host memory.  A file that is not there: an error when it must exist, otherwise an empty `out` and true with no error set
template <class T> static inline bool slurp_file(const std::string &path, std::vector<T> &out, bool must_exist)
{
    out.clear();
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { if (must_exist) harc_set_error("cannot open %s", path.c_str()); return !must_exist; }
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    out.resize((size_t)n);
    const bool ok = n == 0 || fread(out.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    if (!ok) harc_set_error("short read on %s", path.c_str());
    return ok;
}
// Host memory, or a stream of the context, as a whole file
static inline int spit_file(const std::string &path, const void *p, size_t n)
{
    FILE *o = fopen(path.c_str(), "wb");
    if (!o) { harc_set_error("cannot create %s", path.c_str()); return HARC_AMD_EIO; }
    if (n && fwrite(p, 1, n, o) != n) { fclose(o); harc_set_error("short write on %s", path.c_str()); return HARC_AMD_EIO; }
    fclose(o);
    return HARC_AMD_OK;
}
static inline int spit_stream(harc_amd_ctx *c, int id, int shard, const std::string &path)
{
    const void *p = nullptr; size_t n = 0;
    RC_TRY(harc_amd_get_stream(c, id, shard, &p, &n));
    return spit_file(path, p, n);
}
// The output file is removed unless the call reaches its end.  Declare it in front of the FileDrain: it goes after the drain has closed the file
struct OutFileGuard { std::string path; bool ok = false; ~OutFileGuard() { if (!ok) (void)remove(path.c_str()); } };
struct CtxGuard { harc_amd_ctx *c = nullptr; ~CtxGuard() { harc_amd_destroy(c); } };
static inline uint64_t env_u64(const char *name, uint64_t dflt) { if (const char *e = getenv(name)) { const unsigned long long v = strtoull(e, nullptr, 10); if (v >= 1) return v; } return dflt; }
// a context of its own for a call on side files: the default parameters of read length L over *params, the caller's device kept; num_thr: the shards of an archive
static inline int side_context(const harc_amd_params *params, int L, harc_amd_ctx **c, int num_thr = 0)
{
    harc_amd_params P = *params;
    if (harc_amd_default_params(L, &P) != HARC_AMD_OK) return HARC_AMD_EINVAL;
    P.device = params->device;
    if (num_thr) P.num_thr = num_thr;
    // side files of fewer than 4 bases a line: harc:57-60 gives windows of no bases there, which harc_amd_create refuses.  No stage runs on this context
    for (int l = 0; l < 2; l++) if (P.dict_end[l] < P.dict_start[l]) P.dict_end[l] = P.dict_start[l];
    return harc_amd_create(&P, c);
}
// The context's ONE pinned ring in `parts` disjoint parts of `slices_each` slices, out[0 .. parts), for movers that are alive at the same time; the host threads are
// shared out among them.  The ring is reserved whole before any of them starts.  HARC_AMD_FEED_SLICE sets the slice, HARC_AMD_FEED_THREADS the threads of all together.
// slice: the caller's own slice size where the environment names none (spack.hip: files of a few MB do not pin a ring of 1 GiB); 0: the default
static inline int ring_split(harc_amd_ctx *c, int parts, int slices_each, const char *what, RingGeom *out, size_t slice = 0)
{
    RingGeom base;
    if (slice) base.slice = slice;
    harc_ring_geom_env(&base);
    for (int k = 0; k < parts; k++) { out[k].slice = base.slice; out[k].nslices = slices_each; out[k].nthr = base.nthr / parts > 0 ? base.nthr / parts : 1; out[k].ring_off = (size_t)k * slices_each * base.slice; }
    return harc_ring_reserve(c, (size_t)parts * slices_each * base.slice, what);
}
// the `slice` of ring_split for a mover of `slices` slices whose largest piece of work holds `most` bytes: a file of a few MB does not pin a ring of 1 GiB
static inline size_t ring_slice_for(uint64_t most, uint64_t slices)
{
    if (most >= ((uint64_t)16 * 64 << 20)) return 0;
    const uint64_t s = ((most + slices - 1) / slices + 4095) & ~(uint64_t)4095;
    return (size_t)(s < 65536 ? 65536 : s);
}
// What FileFeeder::start takes: the bytes [lo, hi) of a file in pieces of `piece` bytes; n lines of LL bytes each in pieces of `piece_lines` lines
typedef std::vector<std::pair<uint64_t, uint64_t>> Pieces;
static inline Pieces byte_pieces(uint64_t lo, uint64_t hi, uint64_t piece)
{
    Pieces pieces;
    for (uint64_t a = lo; a < hi; a += piece) pieces.emplace_back(a, hi - a < piece ? hi : a + piece);
    return pieces;
}
static inline Pieces line_pieces(uint64_t n, uint64_t LL, uint64_t piece_lines)
{
    Pieces pieces;
    for (uint64_t a = 0; a < n; a += piece_lines) pieces.emplace_back(a * LL, (n - a < piece_lines ? n : a + piece_lines) * LL);
    return pieces;
}

// A device buffer that a file-level call owns and grows piece by piece
struct DevBuf { harc_amd_ctx *c; char *p = nullptr; size_t cap = 0; ~DevBuf() { if (p) harc_raw_free(c, p); } };
// at least `need` bytes, the first `keep` of them kept.  Nothing to keep: the old buffer goes first (the peak stays lower) and the new one is exactly `need`; otherwise
// a quarter more than `need`, and the old one goes when its bytes have been copied
static inline int dev_reserve(DevBuf *b, size_t need, size_t keep = 0)
{
    if (b->p && b->cap >= need) return HARC_AMD_OK;
    harc_amd_ctx *c = b->c;
    if (!keep) {
        HIP_TRY(hipStreamSynchronize(c->stream));                 // whatever still reads the old buffer has finished
        if (b->p) { harc_raw_free(c, b->p); b->p = nullptr; b->cap = 0; }
        RC_TRY(harc_raw_alloc(c, (void **)&b->p, need + 16));
        b->cap = need;
        return HARC_AMD_OK;
    }
    char *np = nullptr; const size_t cap = need + need / 4;
    RC_TRY(harc_raw_alloc(c, (void **)&np, cap + 16));
    hipError_t e = hipMemcpyAsync(np, b->p, keep, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);     // ... and whatever still reads the old buffer has finished
    if (e != hipSuccess) { harc_raw_free(c, np); harc_set_error("growing a device buffer to %zu bytes failed: %s", cap, hipGetErrorString(e)); return HARC_AMD_ENODEVICE; }
    harc_raw_free(c, b->p);
    b->p = np; b->cap = cap;
    return HARC_AMD_OK;
}

// Seconds between two points of a stream, added to *sum; sum == nullptr: every call does nothing.  The events go on every way out
struct KernelTimer {
    double *sum; hipEvent_t e0 = nullptr, e1 = nullptr;
    explicit KernelTimer(double *sum_) : sum(sum_) {}
    KernelTimer(const KernelTimer &) = delete;
    ~KernelTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    int begin(hipStream_t s)
    {
        if (!sum) return HARC_AMD_OK;
        if (!e0) HIP_TRY(hipEventCreate(&e0));
        if (!e1) HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e0, s));
        return HARC_AMD_OK;
    }
    // end() in two halves, for a caller that enqueues more work before it waits
    int end_mark(hipStream_t s) { if (sum) HIP_TRY(hipEventRecord(e1, s)); return HARC_AMD_OK; }
    int end_wait()
    {
        if (!sum) return HARC_AMD_OK;
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1); *sum += 1e-3 * (double)ms;
        return HARC_AMD_OK;
    }
    int end(hipStream_t s) { RC_TRY(end_mark(s)); return end_wait(); }
};

// File -> HBM at the rate of the host's memory system instead of one core's (round 6; round 3's ./harc -c spent most of its 6 s on 100 M reads in a
// single-threaded fread into one pinned buffer): reader threads pread() slices of the file into a ring of pinned slices kept by the context, the calling
// thread uploads every filled slice (hipMemcpyAsync on the context's stream) and hands the slice back when its copy has finished.  The slices of ALL the
// pieces of a range are read ahead in file order as far as the ring goes: while the device indexes and packs piece i the readers already hold the first
// slices of piece i + 1.  A slice is taken from the ring BEFORE its chunk number, under one lock: the chunks that hold slices are always the lowest
// unfinished ones, so a piece being waited for can never starve behind read-ahead that cannot be uploaded yet.
struct FileFeeder {
    struct Chunk { uint64_t off; uint32_t len; uint32_t piece; uint64_t at; };     // file offset, bytes, piece, byte offset inside the piece
    harc_amd_ctx *c; int fd = -1; const char *name;
    bool use_mmap = true;                                         // the readers copy out of a mapping of their slice instead of calling pread (HARC_AMD_FEED_MMAP=0: pread)
    std::vector<Chunk> chunks; std::vector<size_t> piece_left;                     // chunks of each piece not uploaded yet
    size_t SL = 0; int NS = 0; char *ring = nullptr;              // this feeder's part of c->feed_ring
    std::vector<hipEvent_t> ev;
    std::mutex mu; std::condition_variable cv_free, cv_filled;
    std::deque<int> free_slices; std::deque<std::pair<int, size_t>> filled, held;  // (slice, chunk)
    std::deque<int> inflight;                                                      // slices whose upload is on the stream, oldest first
    size_t next_chunk = 0; bool stop = false; int err = 0;
    double t_ring = 0, t_pread = 0, t_wait_free = 0, t_wait_filled = 0, t_wait_copy = 0, t_enqueue = 0;      // HARC_AMD_TRACE: summed over the readers / of the calling thread
    std::vector<std::thread> th;
    FileFeeder(harc_amd_ctx *c_, const char *name_) : c(c_), name(name_) {}
    ~FileFeeder()
    {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv_free.notify_all();
        for (auto &t : th) t.join();
        (void)hipStreamSynchronize(c->stream);                    // before the ring is used again
        if (getenv("HARC_AMD_TRACE")) fprintf(stderr, "[file feeder] %zu slices of %zu MB through %d pinned slices by %zu readers (pinned ring allocated in %.3f s): readers in pread %.2f s, waiting for a free slice %.2f s (summed); uploader enqueueing %.2f s, waiting for a filled slice %.2f s, for a copy %.2f s\n",
                                              chunks.size(), SL >> 20, NS, th.size(), t_ring, t_pread, t_wait_free, t_enqueue, t_wait_filled, t_wait_copy);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (fd >= 0) close(fd);
    }
    // pieces: [lo, hi) byte ranges of the file, in file order
    int start(const std::vector<std::pair<uint64_t, uint64_t>> &pieces, const RingGeom &geom = RingGeom())
    {
        fd = open(name, O_RDONLY);
        if (fd < 0) { harc_set_error("cannot open %s", name); return HARC_AMD_EIO; }
        // 16 slices of 64 MB, 16 readers (tools/micro/feed_rate.cpp, profiles/r06/feed_rate.txt: a file that has been read before reaches HBM at 54 GB/s this way, the
        // PCIe rate is 57; 16-MB slices 42; the FIRST read of a freshly written tmpfs file runs at 24 GB/s whatever is done here -- the kernel's own first touch)
        SL = geom.slice; NS = geom.nslices;
        int nthr = geom.nthr;
        // a read() of page-cache pages that nobody has read yet marks every one of them accessed (LRU lists, under a lock the readers share): the first read of
        // a freshly written 21.7-GB file ran at 14-24 GB/s with 16 readers, the second at 54.  Copies out of a shared mapping do not go that way -- but ONE
        // mapping of the whole file took 0.8 s to take down again (the same marking, at unmap, by one thread): every reader maps its own slice, tells the kernel
        // that it reads it once from front to back (no recency kept for such a mapping), copies and unmaps.  HARC_AMD_FEED_MMAP=0: pread -- the way to read a file
        // that somebody may TRUNCATE meanwhile: a copy out of a mapping beyond the new end of the file is a SIGBUS, not a short read.
        use_mmap = !(getenv("HARC_AMD_FEED_MMAP") && atoi(getenv("HARC_AMD_FEED_MMAP")) == 0);
        const double t_ring0 = mono_now();
        RC_TRY(harc_ring_reserve(c, geom.ring_off + SL * (size_t)NS, "ingest"));
        ring = c->feed_ring + geom.ring_off;
        t_ring = mono_now() - t_ring0;
        ev.assign(NS, nullptr);
        for (int k = 0; k < NS; k++) { if (hipEventCreate(&ev[k]) != hipSuccess) { harc_set_error("hipEventCreate failed"); return HARC_AMD_ENODEVICE; } free_slices.push_back(k); }
        piece_left.assign(pieces.size(), 0);
        for (size_t p = 0; p < pieces.size(); p++)
            for (uint64_t a = pieces[p].first; a < pieces[p].second; a += SL) {
                const uint64_t b = pieces[p].second - a < SL ? pieces[p].second : a + SL;
                chunks.push_back(Chunk{ a, (uint32_t)(b - a), (uint32_t)p, a - pieces[p].first });
                piece_left[p]++;
            }
        if ((size_t)nthr > chunks.size()) nthr = (int)chunks.size();
        for (int t = 0; t < nthr; t++) th.emplace_back([this] { reader(); });
        return HARC_AMD_OK;
    }
    void reader()
    {
        for (;;) {
            int sl; size_t k;
            const double tw0 = mono_now();
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_free.wait(lk, [&] { return stop || next_chunk >= chunks.size() || !free_slices.empty(); });
                if (stop || next_chunk >= chunks.size()) return;
                sl = free_slices.front(); free_slices.pop_front(); k = next_chunk++;
            }
            const Chunk &ch = chunks[k];
            const double tr0 = mono_now();
            char *dst = ring + (size_t)sl * SL; size_t got = 0; int e = 0;
            if (use_mmap) {
                const uint64_t a0 = ch.off & ~(uint64_t)4095; const size_t mlen = (size_t)(ch.off + ch.len - a0);
                void *m = mmap(nullptr, mlen, PROT_READ, MAP_SHARED, fd, (off_t)a0);
                if (m != MAP_FAILED) {
                    (void)madvise(m, mlen, MADV_SEQUENTIAL);
                    memcpy(dst, (const char *)m + (ch.off - a0), ch.len); got = ch.len;
                    munmap(m, mlen);
                }
            }
            while (got < ch.len) {
                const ssize_t r = pread(fd, dst + got, ch.len - got, (off_t)(ch.off + got));
                if (r <= 0) { e = 1; break; }
                got += (size_t)r;
            }
            {
                std::lock_guard<std::mutex> lk(mu);
                if (e) { err = 1; stop = true; }
                filled.emplace_back(sl, k);
                t_wait_free += tr0 - tw0; t_pread += mono_now() - tr0;
            }
            cv_filled.notify_one();
            if (e) { cv_free.notify_all(); return; }
        }
    }
    void give_back(int sl) { { std::lock_guard<std::mutex> lk(mu); free_slices.push_back(sl); } cv_free.notify_one(); }
    // every chunk of piece p on the stream towards d_txt; chunks of piece p + 1 that are ready meanwhile go to d_next (may be null: they wait)
    int upload_piece(size_t p, char *d_txt, char *d_next)
    {
        auto put = [&](int sl, size_t k) -> int {
            const Chunk &ch = chunks[k];
            char *base = ch.piece == p ? d_txt : d_next;
            const double te0 = mono_now();
            if (hipMemcpyAsync(base + ch.at, ring + (size_t)sl * SL, ch.len, hipMemcpyHostToDevice, c->stream) != hipSuccess) { harc_set_error("upload of %s failed", name); return HARC_AMD_ENODEVICE; }
            (void)hipEventRecord(ev[sl], c->stream);
            inflight.push_back(sl); piece_left[ch.piece]--;
            t_enqueue += mono_now() - te0;
            return HARC_AMD_OK;
        };
        // what was read ahead for this piece while the last one was uploaded
        for (size_t i = 0; i < held.size();) {
            const Chunk &ch = chunks[held[i].second];
            if (ch.piece == p || (ch.piece == p + 1 && d_next)) { RC_TRY(put(held[i].first, held[i].second)); held.erase(held.begin() + (long)i); } else i++;
        }
        while (piece_left[p] > 0) {
            while (!inflight.empty() && hipEventQuery(ev[inflight.front()]) == hipSuccess) { give_back(inflight.front()); inflight.pop_front(); }
            std::pair<int, size_t> it(-1, 0);
            {
                std::unique_lock<std::mutex> lk(mu);
                if (filled.empty() && !err) {
                    if (!inflight.empty()) { lk.unlock(); const double t0 = mono_now(); (void)hipEventSynchronize(ev[inflight.front()]); t_wait_copy += mono_now() - t0; give_back(inflight.front()); inflight.pop_front(); continue; }
                    const double t0 = mono_now();
                    cv_filled.wait(lk, [&] { return !filled.empty() || err; });
                    t_wait_filled += mono_now() - t0;
                }
                if (err) { harc_set_error("short read on %s", name); return HARC_AMD_EIO; }
                it = filled.front(); filled.pop_front();
            }
            const Chunk &ch = chunks[it.second];
            if (ch.piece == p || (ch.piece == p + 1 && d_next)) RC_TRY(put(it.first, it.second));
            else held.push_back(it);
        }
        return HARC_AMD_OK;
    }
};

// HBM -> file at the rate of the host's memory system (round 6: decoder.out's replacement spent 4.4 of its 4.7 s on 100 M reads in D2H copies into pageable
// vectors and one thread's fwrite): the output file is sized and mapped first (its length is known from the stream files' sizes), the calling thread sends
// pieces of device memory through a ring of pinned slices (hipMemcpyAsync on the context's stream), writer threads copy every slice that has arrived into the
// mapping.  write() calls to ONE tmpfs file serialise on its inode (tools/micro/feed_rate.cpp: 6 GB/s with 1 or 16 threads); page faults of a shared mapping do not.
struct FileDrain {
    struct Job { int sl; size_t len; uint64_t off; };
    harc_amd_ctx *c; int fd = -1; char *map = nullptr; size_t fsize = 0;
    size_t SL = 0; int NS = 0; char *ring = nullptr;              // this drain's part of c->feed_ring
    std::vector<hipEvent_t> ev;
    std::mutex mu; std::condition_variable cv_free, cv_job, cv_idle;
    std::deque<int> free_slices; std::deque<Job> jobs; int busy = 0; bool stop = false;
    std::vector<std::thread> th;
    // the file's blocks are ALLOCATED ahead of the writers by a thread of its own (posix_fallocate, 64 MB at a time): a store into a mapping of a sparse file on a full
    // file system is a SIGBUS, not an error code -- this way "no space left" is an error of the call, as it was with fwrite
    std::thread alloc_th; std::condition_variable cv_alloc; uint64_t alloc_upto = 0; int alloc_err = 0;
    // a file whose size is only bounded when it is opened (BGZF output): `bytes` of start() is the bound, blocks are allocated no further than what put() has been
    // given (lazy), and finish() cuts the file to the size set_final_size() announced
    std::condition_variable cv_goal; uint64_t alloc_goal = 0; bool lazy = false; bool have_final = false; uint64_t final_size = 0;
    std::string fname;
    explicit FileDrain(harc_amd_ctx *c_) : c(c_) {}
    ~FileDrain() { (void)finish(); }
    // geom == nullptr: the whole ring in the default geometry, with HARC_AMD_FEED_SLICE / HARC_AMD_FEED_THREADS read here
    void set_final_size(uint64_t n) { have_final = true; final_size = n; }
    void raise_goal(uint64_t upto) { if (!lazy) return; { std::lock_guard<std::mutex> lk(mu); if (upto > alloc_goal) alloc_goal = upto; } cv_goal.notify_all(); }
    int start(const std::string &path, size_t bytes, const RingGeom *geom = nullptr, bool lazy_alloc = false)
    {
        lazy = lazy_alloc; alloc_goal = lazy_alloc ? 0 : (uint64_t)bytes;
        fd = open(path.c_str(), O_CREAT | O_RDWR | O_TRUNC, 0644);
        if (fd < 0) { harc_set_error("cannot create %s", path.c_str()); return HARC_AMD_EIO; }
        fsize = bytes; fname = path;
        if (bytes) {
            if (ftruncate(fd, (off_t)bytes) != 0) { harc_set_error("cannot size %s to %zu bytes", path.c_str(), bytes); return HARC_AMD_EIO; }
            map = (char *)mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
            if (map == MAP_FAILED) { map = nullptr; harc_set_error("cannot map %s", path.c_str()); return HARC_AMD_EIO; }
        }
        RingGeom g;
        if (geom) g = *geom; else harc_ring_geom_env(&g);
        SL = g.slice; NS = g.nslices;
        const int nthr = g.nthr;
        RC_TRY(harc_ring_reserve(c, g.ring_off + SL * (size_t)NS, "output"));
        ring = c->feed_ring + g.ring_off;
        ev.assign(NS, nullptr);
        for (int k = 0; k < NS; k++) { if (hipEventCreate(&ev[k]) != hipSuccess) { harc_set_error("hipEventCreate failed"); return HARC_AMD_ENODEVICE; } free_slices.push_back(k); }
        alloc_th = std::thread([this] {
            const uint64_t STEP = (uint64_t)64 << 20;
            for (uint64_t a = 0; a < (uint64_t)fsize; a += STEP) {
                if (lazy) { std::unique_lock<std::mutex> lk(mu); cv_goal.wait(lk, [&] { return stop || alloc_goal > a; }); if (alloc_goal <= a) break; }
                const uint64_t len = (uint64_t)fsize - a < STEP ? (uint64_t)fsize - a : STEP;
                const int e = posix_fallocate(fd, (off_t)a, (off_t)len);
                std::lock_guard<std::mutex> lk(mu);
                if (e == EOPNOTSUPP || e == EINVAL) { alloc_upto = (uint64_t)fsize; break; }      // a file system without preallocation: as before this round
                if (e) { alloc_err = e; break; }
                alloc_upto = a + len;
                cv_alloc.notify_all();
                if (stop) break;
            }
            cv_alloc.notify_all();
        });
        const int dev = c->P.device;
        for (int t = 0; t < nthr; t++) th.emplace_back([this, dev] {
            (void)hipSetDevice(dev);
            for (;;) {
                Job j;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv_job.wait(lk, [&] { return stop || !jobs.empty(); });
                    if (jobs.empty()) return;
                    j = jobs.front(); jobs.pop_front(); busy++;
                }
                (void)hipEventSynchronize(ev[j.sl]);              // the slice has arrived
                bool space;
                { std::unique_lock<std::mutex> lk(mu); cv_alloc.wait(lk, [&] { return alloc_err != 0 || alloc_upto >= j.off + j.len; }); space = alloc_err == 0; }
                if (space) memcpy(map + j.off, ring + (size_t)j.sl * SL, j.len);
                { std::lock_guard<std::mutex> lk(mu); busy--; free_slices.push_back(j.sl); }
                cv_free.notify_one(); cv_idle.notify_all();
            }
        });
        return HARC_AMD_OK;
    }
    // n bytes of device memory -> bytes [off, off + n) of the file.  The copies are on the context's stream: what is enqueued behind them may reuse d_src
    int put(const void *d_src, size_t n, uint64_t off)
    {
        if (off + n > fsize) { harc_set_error("output file: %zu bytes at %llu do not fit its %zu bytes", n, (unsigned long long)off, fsize); return HARC_AMD_EINTERNAL; }
        raise_goal(off + n);
        for (size_t a = 0; a < n; a += SL) {
            const size_t len = n - a < SL ? n - a : SL;
            int sl;
            { std::unique_lock<std::mutex> lk(mu); cv_free.wait(lk, [&] { return !free_slices.empty(); }); sl = free_slices.front(); free_slices.pop_front(); }
            if (hipMemcpyAsync(ring + (size_t)sl * SL, (const char *)d_src + a, len, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipEventRecord(ev[sl], c->stream) != hipSuccess) {
                harc_set_error("device -> host copy of the output failed"); return HARC_AMD_ENODEVICE; }
            { std::lock_guard<std::mutex> lk(mu); jobs.push_back(Job{ sl, len, off + a }); }
            cv_job.notify_one();
        }
        return HARC_AMD_OK;
    }
    int put_host(const void *h, size_t n, uint64_t off)
    {
        if (off + n > fsize) { harc_set_error("output file: %zu bytes at %llu do not fit its %zu bytes", n, (unsigned long long)off, fsize); return HARC_AMD_EINTERNAL; }
        raise_goal(off + n);
        if (n) {
            { std::unique_lock<std::mutex> lk(mu); cv_alloc.wait(lk, [&] { return alloc_err != 0 || alloc_upto >= off + n; }); if (alloc_err) return HARC_AMD_OK; }      // (finish() reports it)
            memcpy(map + off, h, n);
        }
        return HARC_AMD_OK;
    }
    int finish()
    {
        if (!th.empty()) {
            { std::unique_lock<std::mutex> lk(mu); cv_idle.wait(lk, [&] { return jobs.empty() && busy == 0; }); stop = true; }
            cv_job.notify_all();
            for (auto &t : th) t.join();
            th.clear();
        }
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv_goal.notify_all();
        if (alloc_th.joinable()) alloc_th.join();
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        ev.clear();
        if (map) { munmap(map, fsize); map = nullptr; }
        bool cut_failed = false;
        if (fd >= 0) { if (have_final && final_size < fsize && ftruncate(fd, (off_t)final_size) != 0) cut_failed = true; close(fd); fd = -1; }
        if (cut_failed) { harc_set_error("cannot cut %s to its %llu bytes", fname.c_str(), (unsigned long long)final_size); return HARC_AMD_EIO; }
        if (alloc_err) { harc_set_error("cannot allocate %zu bytes for %s: %s", fsize, fname.c_str(), strerror(alloc_err)); const int e = alloc_err; alloc_err = 0; (void)e; return HARC_AMD_EIO; }
        return HARC_AMD_OK;
    }
};

// A text that arrives in pieces and is worked in whole units (lines, blocks): what lies behind the last whole unit of a piece is carried to the front of the next.
// Two buffers take turns: the carried bytes are copied device to device on the stream, behind the kernels that still read the piece they are cut from.
// One turn over the lines of the text at hand: text[0 .. total) holds `lines` lines by the index nls, the last of them without its newline when `open`; the first
// `whole` of them are worked in this turn and end in front of byte `cut`.  line0: whole lines of the turns before (walk_lines); stop: end_at() was called
struct LineTurn { char *text; const uint64_t *nls; uint64_t total, lines, whole, cut, line0; bool open, stop; };
struct CarriedText {
    DevBuf buf[2]; int cur = 0; uint64_t carry = 0;               // carry: bytes at the front of text() that the last piece left
    explicit CarriedText(harc_amd_ctx *c) : buf{ { c }, { c } } {}
    char *text() const { return buf[cur].p; }
    // piece p of the feeder, `len` bytes, behind what was carried: text()[0 .. carry + len).  *t_read: seconds in the upload
    int take(FileFeeder &feed, size_t p, uint64_t len, double *t_read)
    {
        RC_TRY(dev_reserve(&buf[cur], (size_t)(carry + len), (size_t)carry));
        const double t0 = mono_now();
        RC_TRY(feed.upload_piece(p, buf[cur].p + carry, nullptr));
        *t_read += mono_now() - t0;
        return HARC_AMD_OK;
    }
    // the `rest` bytes from byte `cut` of text() on are carried: they become the front of the other buffer
    int carry_from(uint64_t cut, uint64_t rest)
    {
        RC_TRY(dev_reserve(&buf[cur ^ 1], (size_t)rest));
        HIP_TRY(hipMemcpyAsync(buf[cur ^ 1].p, buf[cur].p + cut, (size_t)rest, hipMemcpyDeviceToDevice, buf[cur].c->stream));
        cur ^= 1; carry = rest;
        return HARC_AMD_OK;
    }
    // ---- the steps of a turn over whole lines
    // the lines of text()[0 .. total).  An open last line is a whole line only where the file ends (`last`).  Pool memory: the caller brackets the turn
    int index(uint64_t total, bool last, LineTurn *t)
    {
        t->text = text(); t->total = t->cut = total; t->line0 = 0; t->stop = false;
        RC_TRY(text_line_index(buf[0].c, t->text, total, &t->nls, &t->lines, &t->open));
        t->whole = t->lines - ((t->open && !last) ? 1 : 0);
        return HARC_AMD_OK;
    }
    // *at: the byte behind line k - 1, where line k starts (of lines that have their newline)
    int line_end(const uint64_t *nls, uint64_t k, uint64_t *at)
    {
        *at = 0;
        if (!k) return HARC_AMD_OK;
        hipStream_t s = buf[0].c->stream;
        HIP_TRY(hipMemcpyAsync(at, nls + (k - 1), 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        *at += 1;
        return HARC_AMD_OK;
    }
    // a walk's callable takes the first m <= whole lines of the turn only, and the walk ends behind them
    int end_at(LineTurn *t, uint64_t m)
    {
        t->stop = true;
        if (m == t->whole) return HARC_AMD_OK;
        t->whole = m;
        return line_end(t->nls, m, &t->cut);
    }
    // what lies behind byte `cut` of the `total` at hand is carried; with no whole unit in front of it the text stays where it is and grows by the next piece
    int carry_behind(uint64_t cut, uint64_t total)
    {
        if (total - cut && cut) return carry_from(cut, total - cut);
        carry = total - cut;
        return HARC_AMD_OK;
    }
};

// The gather of a selection's files (select.hip: harc_gather_files; -L and -M share it).  flags: device memory, 0 or 1 a line of the reads' file, and where there is
// an id file the first id_lines of them are the id lines' flags.  ids_path / quality_path may be null: that text is not part of the job and its output is not written.
// out_lines: the flagged lines of the reads' file.  feed, drain: disjoint parts of the context's ring
struct GatherFiles {
    const char *who = "", *ids_path = nullptr, *dna_path = nullptr, *quality_path = nullptr, *out_ids_path = nullptr, *out_dna_path = nullptr, *out_quality_path = nullptr;
    uint64_t isz = 0, id_lines = 0, reads = 0, S = 0, out_lines = 0; const uint8_t *flags = nullptr; RingGeom feed, drain; LapTimer *lap = nullptr;
    bool ids_counted = true;                                      // the caller has walked the id file and found id_lines lines; false: the gather's walk is the first to count them
};
int harc_gather_files(harc_amd_ctx *c, const GatherFiles &J);
int harc_flags_or_halves(harc_amd_ctx *c, uint8_t *f, uint64_t n);
int harc_flags_count(harc_amd_ctx *c, const uint8_t *p, uint64_t n, uint64_t *out);

// How walk_lines goes through the bytes [begin, fsz) of a file of lines of any length in pieces of `piece` bytes, and what it found.  text_limit: a text at hand
// (what is carried and the piece) of more bytes is refused (0: any); sync_turn: the stream is waited for before a turn's line index goes
struct LineWalk {
    uint64_t begin = 0, piece = 0; RingGeom geom; uint64_t text_limit = 0; bool sync_turn = false;
    uint64_t lines = 0, end = 0; double t_read = 0;               // out: the whole lines of all turns, the byte of the file behind the last of them, seconds in the uploads
};
// Every turn hands the whole lines of the text at hand to work(txt, turn): what lies behind a piece's last whole line is carried, a piece without a whole line grows
// by the next one, and the last line of the file counts as a line with or without its newline.  work may cut the walk short (CarriedText::end_at)
template <class F> static int walk_lines(harc_amd_ctx *c, const char *path, uint64_t fsz, LineWalk *w, F work)
{
    w->lines = 0; w->end = w->begin;
    const Pieces pieces = byte_pieces(w->begin, fsz, w->piece);
    if (pieces.empty()) return HARC_AMD_OK;
    CarriedText txt(c);
    FileFeeder feed(c, path);                                     // (goes first, and waits for the stream: nothing reads the text any more when its buffers go)
    RC_TRY(feed.start(pieces, w->geom));
    for (size_t p = 0; p < pieces.size(); p++) {
        const uint64_t len = pieces[p].second - pieces[p].first, total = txt.carry + len, origin = pieces[p].first - txt.carry;
        if (w->text_limit && total > w->text_limit) { harc_set_error("%s: a line of more than %llu bytes", path, (unsigned long long)(total - len)); return HARC_AMD_EINVAL; }
        RC_TRY(txt.take(feed, p, len, &w->t_read));
        PoolScope turn(c);
        LineTurn t;
        RC_TRY(txt.index(total, p + 1 == pieces.size(), &t));
        t.line0 = w->lines;
        if (t.whole < t.lines) RC_TRY(txt.line_end(t.nls, t.whole, &t.cut));
        if (t.whole) RC_TRY(work(txt, t));
        w->lines += t.whole; w->end = origin + t.cut;
        if (t.stop) break;
        RC_TRY(txt.carry_behind(t.cut, total));
        if (w->sync_turn) HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return HARC_AMD_OK;
}
