/*
 * harc_amd.h -- C-ABI of libharc_amd.so: the MI355X (gfx950) implementation of HARC's hash-based read reordering
 * + reference-delta encoding hot path.  Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * What each entry point replaces in the reference (file:line into shubhamchandak94/HARC):
 *
 *   harc_amd_reorder_files     == `reorder.out <basedir>`      src/reorder.cpp:100-131, invoked at harc:67
 *   harc_amd_encoder_files     == `encoder.out <basedir>`      src/encoder.cpp:108-152, invoked at harc:69
 *   harc_amd_pack_order_files  == `pack_order.out <basedir>`   src/pack_order.cpp:11-18, invoked at harc:112
 *   harc_amd_compress_files    == harc:65-69 fused (stage I -> stage II handed over in HBM, no temp.dna round trip)
 *   harc_amd_params            == the compile-time macros the bash driver writes to src/config.h (harc:52-63)
 *
 *   In-memory API (what a cgo/JNI/ctypes binding of the same path would bind; used by bench.py and the tests):
 *   harc_amd_create/destroy, harc_amd_set_* (inputs = what reorder.cpp:240-263 readDnaFile / encoder.cpp:823-872
 *   readsingletons parse), harc_amd_reorder (reorder.cpp:277-703), harc_amd_encode (encoder.cpp:154-616),
 *   harc_amd_pack_order (pack_order.cpp:20-77), harc_amd_get_stream (the files of reorder.cpp:722-830 and
 *   encoder.cpp:190-196,457-503 as byte ranges).
 *
 * Conventions: every function returns 0 on success, a negative HARC_AMD_E* code otherwise (the reference's
 * programs return 0 / print a message; the bash driver runs under `set -e`, harc:2).  No exceptions cross the ABI.
 * Input buffers are caller-owned and may be released after the call returns.  Device input buffers must be COMPLETE when
 * the call is made: the library works on its own HIP stream and does not wait for the caller's streams.  Output buffers returned by
 * harc_amd_get_stream are library-owned host memory, valid until the next harc_amd_reorder/encode/pack_order on
 * the same context or harc_amd_destroy.  One context per host thread; one HIP device per context.
 *
 * There is NO CPU fallback: every compute entry point fails with HARC_AMD_ENODEVICE when no gfx950 device is usable.
 */
#ifndef HARC_AMD_H
#define HARC_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HARC_AMD_OK 0
#define HARC_AMD_EINVAL (-1)      /* bad argument / parameter out of range (readlen > 255: harc:46-49, preprocess.cpp:122) */
#define HARC_AMD_ENODEVICE (-2)   /* no usable HIP device, or a HIP call failed (message via harc_amd_last_error) */
#define HARC_AMD_EIO (-3)         /* file contract violated (missing / short file) */
#define HARC_AMD_ESTATE (-4)      /* call order violated (e.g. encode before reorder and without stage-I inputs) */
#define HARC_AMD_ENOMEM (-5)
#define HARC_AMD_ETIMEOUT (-7)    /* multi-GPU: the peers did not answer a collective within HARC_AMD_COMM_TIMEOUT seconds (default 600); the communicator is gone */
#define HARC_AMD_EINTERNAL (-6)    /* an invariant of the library failed (bookkeeping mismatch, a schedule that does not settle): a bug, not an input problem */

/* Runtime equivalent of src/config.h (harc:52-63).  Fill with harc_amd_default_params, then override. */
typedef struct harc_amd_params {
    int32_t readlen;          /* `readlen`; 1..255 */
    int32_t num_thr;          /* `num_thr`: E, the number of encoder shards; visible in the output file suffixes (encoder.cpp:190-196) */
    int32_t num_chains;       /* K concurrent chains of stage I.  1 reproduces the reference at num_thr=1 byte for byte.
                                 0 = auto (throughput mode).  The reference's own num_thr>1 is a race (reorder.cpp:545-552);
                                 K>1 here is the deterministic round-synchronous schedule documented in DESIGN.md. */
    int32_t maxmatch;         /* `maxmatch` = readlen/2; accepted: 0 .. min(128, readlen) */
    int32_t thresh;           /* `thresh` = 4; accepted: >= 0 */
    int32_t thresh_s;         /* `thresh_s` = 24; accepted: >= 0 */
    int32_t maxsearch;        /* `maxsearch` = 1000; accepted: >= 1 */
    int32_t dict_start[2];    /* `dict1_start`,`dict2_start` */
    int32_t dict_end[2];      /* `dict1_end`,`dict2_end`: each window 1 .. 32 bases inside the read, anywhere, in any order, overlapping or not.  A window of no
                                 bases (dict_end = dict_start - 1) is refused with HARC_AMD_EINVAL: it has no meaning in the reference.  (harc:57-60 gives such
                                 windows below 4 bases: harc_amd_default_params fills them in, harc_amd_create refuses them.) */
    int32_t device;           /* HIP device ordinal */
    int32_t profile;          /* 1: time every launch of the dominant kernel with HIP events on the context's stream */
    int32_t num_steps;        /* S: speculative chain steps per launch of the chain kernel (1..64; 0 = auto: 16; 64 for one chain; 32 from
                                 16 385 chains on -- and from 2048 chains on where the input is not a low-coverage one (at most 98 % of the reads
                                 alone in their first-dictionary bin) -- where the index's bins of more than 16 reads hold at most 2 % of N
                                 entries: a function of the input alone).  Output is independent of S when num_chains = 1; for num_chains > 1
                                 the pair (K,S) defines the schedule */
    int32_t reads_per_chain;  /* auto mode (num_chains = 0): one chain per this many reads, capped at 65536 chains; 0 = 2048 (inputs below 4 M reads:
                                 up to 2048 chains of at least 1024 reads; low-coverage ones up to 4096 of at least 256).  Inputs that are
                                 already fragmented (one minimizer bucket of a multi-GPU shard) lose nothing with 1024 and run faster. */
    int32_t decode_memory_gb; /* -m of `./harc -d -p` (harc:225, MAX_BIN_SIZE of decoder_preserve.cpp:249-253): the original order is restored in bins of
                                 decode_memory_gb * 2e8 / 7 reads (0 = the driver's default 7; <= 3 counts as 3), and never more than fits in HBM */
    int32_t stream_digest;    /* 1: harc_amd_encode also folds every stage-II stream into four 64-bit words where it sits in HBM (harc_amd_stream_digest):
                                 two runs, two kernel variants or two GPUs are compared at full size without touching gigabytes of host memory */
    int32_t table_slots_per_read; /* 16-byte slots per read in each of the two stage-I dictionaries (the replacement of BooPHF.h's MPHF + startpos, reorder.cpp:277-394):
                                 4, 3 or 2; 0 = the library chooses -- 4 while one table stays below 15 % of the device's memory and a fifth of what is free, else 3,
                                 else 2.  A memory / speed choice, not visible in any output byte: configs[3] on one GPU 167 / 149 / 142 GB at 100 / 98.6 / 95.5 %
                                 of the speed (206 / 184 / 176 bytes per input read) */
} harc_amd_params;

/* Counters: the three numbers the reference prints (reorder.cpp:701, encoder.cpp:506-508) + kernel-side statistics. */
typedef struct harc_amd_counters {
    uint64_t n_clean, n_N;            /* inputs */
    uint64_t n_main, n_singleton;     /* stage I: reads in temp.dna / temp.dna.singleton */
    uint64_t unmatched;               /* "Reordering done, X were unmatched" */
    uint64_t aligned_singletons;      /* "X singleton reads were aligned" */
    uint64_t aligned_N;               /* "X reads with N were aligned" */
    uint64_t chains, rounds;          /* stage I schedule */
    uint64_t probes;                  /* hash-table slots inspected by the chain kernel */
    uint64_t candidates;              /* candidate reads fetched + Hamming-tested by the chain kernel */
    uint64_t conflicts;               /* proposals that lost arbitration */
    uint64_t propose_launches;        /* launches of k_steps' main form (the cooperative kernel not included) */
    double propose_ms;                /* sum of their HIP-event durations (params.profile=1), else 0 */
    double index_ms, chain_ms, encode_ms, total_ms;   /* host wall-clock of the phases, stream-synchronised */
    uint64_t contigs, seq_bases;      /* stage II */
    uint64_t bins_over_maxsearch;     /* stage-II dictionary bins larger than maxsearch: their probes are replayed sequentially
                                         (sliding window of encoder.cpp:293, exact) */
    uint64_t device_bytes_peak;
    uint64_t useful_probes;           /* dictionary keys a strictly sequential scan (reorder.cpp:517-649) would have looked up:
                                         priority index of the winning probe + 1, or all probes of the step on a miss */
    uint64_t candidates_seq;          /* candidates that sequential scan would have fetched and Hamming-tested: those of the probes up to and
                                         including the winning one (`candidates` also counts the speculative ones behind it) */
    /* the two kernels of the chain phase apart (round 6): the main kernel's launches are propose_launches / propose_ms; walks that reach a dictionary
       bin of more than 16 reads (repeat families: up to maxsearch Hamming tests per probe, reorder.cpp:540-556) go through the cooperative kernel,
       whose scans stream bin-ordered mirrors of the reads out of L2 -- another ceiling than the main kernel's random accesses */
    uint64_t coop_launches; double coop_ms;
    uint64_t coop_useful_probes, coop_candidates_seq, coop_candidates;   /* its share of useful_probes / candidates_seq / candidates */
    uint64_t coop_steps, dense_steps; /* chain steps WALKED by the launches of either kernel (kept or rolled back) */
} harc_amd_counters;

/* stream ids for harc_amd_get_stream; names are the reference's file names */
enum {
    /* stage I (reorder.cpp:722-830); shard must be 0 */
    HARC_AMD_S1_ORDER = 0,          /* read_order.bin            u32 per main read */
    HARC_AMD_S1_FLAG = 1,           /* tempflag.txt              '0'/'1' */
    HARC_AMD_S1_POS = 2,            /* temppos.txt               u8 */
    HARC_AMD_S1_RC = 3,             /* read_rev.txt              'd'/'r' */
    HARC_AMD_S1_ORDER_SINGLETON = 4,/* read_order.bin.singleton  u32 */
    HARC_AMD_S1_DNA = 5,            /* temp.dna                  text, produced on demand */
    HARC_AMD_S1_DNA_SINGLETON = 6,  /* temp.dna.singleton        text, produced on demand */
    /* stage II (encoder.cpp); per shard e in [0,num_thr) */
    HARC_AMD_S2_SEQ = 10,           /* read_seq.txt.<e>      2-bit packed */
    HARC_AMD_S2_SEQ_TAIL = 11,      /* read_seq.txt.<e>.tail */
    HARC_AMD_S2_POS = 12,           /* read_pos.txt.<e> */
    HARC_AMD_S2_NOISE = 13,         /* read_noise.txt.<e> */
    HARC_AMD_S2_NOISEPOS = 14,      /* read_noisepos.txt.<e> */
    HARC_AMD_S2_REV = 15,           /* read_rev.txt.<e>      1-bit packed */
    HARC_AMD_S2_REV_TAIL = 16,      /* read_rev.txt.<e>.tail */
    /* stage II, whole job; shard must be 0 */
    HARC_AMD_S2_ORDER = 20,         /* read_order.bin (post-encode; encoder.cpp:458-500) */
    HARC_AMD_S2_ORDER_N_PE = 21,    /* read_order_N_pe.bin */
    HARC_AMD_S2_SINGLETON = 22,     /* read_singleton.txt    2-bit packed */
    HARC_AMD_S2_SINGLETON_TAIL = 23,/* read_singleton.txt.tail */
    HARC_AMD_S2_INPUT_N = 24,       /* input_N.dna rewritten: unaligned N reads (encoder.cpp:493-499) */
    HARC_AMD_S2_META = 25,          /* read_meta.txt */
    /* -p (pack_order.cpp) */
    HARC_AMD_P_ORDER = 30,          /* read_order.bin packed */
    HARC_AMD_P_ORDER_TAIL = 31,     /* read_order.bin.tail */
    /* FASTQ ingest (preprocess.cpp:102) */
    HARC_AMD_IN_ORDER_N = 40        /* read_order_N.bin: original index (u32) of every read with N, after harc_amd_set_fastq_device */
};

typedef struct harc_amd_ctx harc_amd_ctx;

/* harc:52-60 formulae.  num_thr=8 (harc:195), num_chains=0 (auto). */
int harc_amd_default_params(int32_t readlen, harc_amd_params *out);

int harc_amd_create(const harc_amd_params *params, harc_amd_ctx **out);
void harc_amd_destroy(harc_amd_ctx *ctx);
const char *harc_amd_last_error(void);

/* ---- inputs.  Clean reads = the lines of input_clean.dna (alphabet ACGT, preprocess.cpp:104-108). */
/* host ASCII; read i starts at ascii + i*stride (stride = readlen+1 for the file layout, reorder.cpp:252) */
int harc_amd_set_reads_ascii(harc_amd_ctx *ctx, const char *ascii, uint32_t n_reads, uint32_t stride);
/* same, buffer already in device memory of params.device */
int harc_amd_set_reads_ascii_device(harc_amd_ctx *ctx, const char *d_ascii, uint32_t n_reads, uint32_t stride);
/* device buffer of n_reads * ceil(2*readlen/64) little-endian u64 words in std::bitset<2*readlen> layout
   (reorder.cpp:184-198: base i at bits 2i,2i+1, A=0 G=1 C=2 T=3); the buffer is copied */
int harc_amd_set_reads_packed_device(harc_amd_ctx *ctx, const uint64_t *d_packed, uint32_t n_reads);
/* reads containing N = the lines of input_N.dna (preprocess.cpp:98-103); host ASCII */
int harc_amd_set_nreads_ascii(harc_amd_ctx *ctx, const char *ascii, uint32_t n_reads, uint32_t stride);
int harc_amd_set_nreads_ascii_device(harc_amd_ctx *ctx, const char *d_ascii, uint32_t n_reads, uint32_t stride);
/* FASTQ text (4-line records) already in device memory: preprocess.cpp:81-121 + readDnaFile on the GPU -- takes line 2 of every
   record, checks the fixed read length, packs reads without N into the 2-bit store and reads with N into the 3-bit store; the
   original indices of the N reads become stream HARC_AMD_IN_ORDER_N.  Replaces harc_amd_set_reads_* + harc_amd_set_nreads_*. */
int harc_amd_set_fastq_device(harc_amd_ctx *ctx, const char *d_fastq, uint64_t n_bytes, uint64_t *n_records_out);
/* BGZF bytes (SAM/BAM spec 4.1: gzip members carrying a BC subfield) in device memory -> their text in device memory, inflated on the GPU.
   d_out == NULL: *n_out = size of the text (sum of ISIZE), nothing decoded; else out_capacity must be at least that.  A chain of members that
   leaves the buffer, a position where a member must start but none parses, ISIZE > 65536, a wrong length or CRC-32 or malformed DEFLATE
   data: HARC_AMD_EINVAL naming the compressed byte offset of the member. */
int harc_amd_bgzf_inflate_device(harc_amd_ctx *ctx, const uint8_t *d_bgzf, uint64_t n_bytes, char *d_out, uint64_t out_capacity, uint64_t *n_out);
/* ---- Any gzip file (RFC 1952: one DEFLATE stream per member, what gzip, sequencer software and fastq-dump --gzip write) inflated on the GPU.  A stream has no
   member table to cut it by: the compressed bytes are cut into chunks (256 KiB; HARC_AMD_GUNZIP_CHUNK=bytes, at least 64, or chunk_bytes where a call takes
   it; 0 = the default), a kernel finds in every chunk the first bit offset at which a non-final dynamic block header parses, every such start is decoded to the
   end of its chunk with the 32 KiB window in front of it kept symbolic, the host chains the walks (a walk whose start the chain does not land on is dropped;
   where the chain lands on no start, one walk is counted from there: a repair), the windows are resolved in file order and the symbols translated, CRC-32 and
   ISIZE of every member checked.  harc_amd/csrc/inflate_stream.h holds the rules, NOTES.md (Plain gzip input) what it measures. */
typedef struct harc_amd_gunzip_stats {
    uint64_t members;          /* gzip members */
    uint64_t chunks;           /* chunks looked at, summed over members (and over pieces of a file) */
    uint64_t starts_found;     /* chunks behind a first one in which the finder found a start */
    uint64_t starts_dropped;   /* of them: never reached by the chain, or not decodable */
    uint64_t repair_walks;     /* walks counted one at a time because the chain landed on no start */
    uint64_t text_bytes;
} harc_amd_gunzip_stats;
/* gzip bytes in device memory -> their text in device memory.  d_out == NULL: *n_out = size of the text, nothing written (the members are walked to learn
   it, their CRC-32 is not checked); else out_capacity must be at least that, and no byte outside [d_out, d_out + *n_out) is written.  Damaged input --
   no gzip header, malformed DEFLATE data, input that ends inside a block or a trailer, a wrong CRC-32 or ISIZE, anything behind a trailer that is no member
   header (zero padding included) -- is HARC_AMD_EINVAL naming the compressed byte.  stats may be NULL. */
int harc_amd_gunzip_device(harc_amd_ctx *ctx, const uint8_t *d_gz, uint64_t n_bytes, uint64_t chunk_bytes, char *d_out, uint64_t out_capacity, uint64_t *n_out,
                           harc_amd_gunzip_stats *stats);
/* the same chunked algorithm run in a row on the host (host memory, no device): the same text, the same stats, the same refusals (tests) */
int harc_amd_gunzip_host(const uint8_t *gz, uint64_t n_bytes, uint64_t chunk_bytes, char *out, uint64_t out_capacity, uint64_t *n_out, harc_amd_gunzip_stats *stats);
/* gz_path -> out_path, inflated on the GPU; only `device` is taken from params.  The compressed file runs through the pinned ring in pieces (64 MiB;
   HARC_AMD_GUNZIP_PIECE=bytes in tests); what lies behind the last block boundary reached in a piece is carried into the next with the boundary's bit offset and
   the resolved window, so the file may be larger than device memory, and the text of one piece that would not fit HARC_AMD_GUNZIP_BUDGET bytes (1 GiB) is
   produced in several turns.  On any failure out_path is removed.  HARC_AMD_TRACE=1 laps the stages on stderr. */
int harc_amd_gunzip_files(const harc_amd_params *params, const char *gz_path, const char *out_path, harc_amd_gunzip_stats *stats);
/* The other way: text in device memory -> BGZF in device memory, deflated on the GPU. The text is cut every 65 280 bytes (bgzip's size) into members that are
   deflated independently, a workgroup each: matches only against the line four lines up at the same column (what repeats in FASTQ; no search), one dynamic
   Huffman block per member, a stored block where that is not smaller (harc_amd/csrc/deflate_member.h holds the rules).  The bytes depend on the text alone.
   flags bit 0: the 28-byte end-of-file marker follows the last member; n_bytes == 0 gives the marker alone, or nothing.  *n_out = bytes of the members (and the
   marker).  d_out == NULL: the size alone (the members are deflated to learn it); else HARC_AMD_EINVAL naming both numbers when out_capacity is smaller.
   harc_amd_bgzf_bound(n_bytes) is always enough.  No byte outside [d_out, d_out + *n_out) is written, whatever the alignment of d_out or d_text. */
uint64_t harc_amd_bgzf_bound(uint64_t n_text);        /* host only: ceil(n / 65280) * (65280 + 31) + 28 */
int harc_amd_bgzf_deflate_device(harc_amd_ctx *ctx, const char *d_text, uint64_t n_bytes, int32_t flags, uint8_t *d_out, uint64_t out_capacity, uint64_t *n_out);
/* the same encoder run in a row on the host (host memory, no device): what the kernels must write, byte for byte.  out_capacity >= harc_amd_bgzf_bound(n_bytes) */
int harc_amd_bgzf_deflate_host(const char *text, uint64_t n_bytes, int32_t flags, uint8_t *out, uint64_t out_capacity, uint64_t *n_out);
/* The way back to FASTQ: n_records ids (d_ids: id_bytes of text, one id per line, any length, 0 included; a last line without its newline counts as a
   line), reads and quality values (d_dna, d_quality: n_records lines at a stride of readlen + 1, readlen 1..255 whatever the context's own read length
   is), all in device memory -> the records  id_i \n read_i \n + \n quality_i \n  at d_out.  The third line is a bare '+' in this call; where every third line of the
   input repeated its id, harc_amd_fastq_assemble_third_device writes that form back (below, "Third lines").  *n_out = id_bytes (+ 1 if the last id lacks its newline) + n_records * (2 * readlen + 4).
   d_out == NULL: the inputs are validated and the size returned, nothing written; else out_capacity must be at least that.
   HARC_AMD_EINVAL, with the counts in harc_amd_last_error(): the id text does not hold exactly n_records lines; a byte at a (readlen + 1)-stride position
   of the reads or the quality values is no newline, or a newline sits anywhere else in them (counted on the device; what was written to d_out by
   then is unspecified); out_capacity is too small. */
int harc_amd_fastq_assemble_device(harc_amd_ctx *ctx, const char *d_ids, uint64_t id_bytes, const char *d_dna, const char *d_quality, uint32_t n_records,
                                   int32_t readlen, char *d_out, uint64_t out_capacity, uint64_t *n_out);
/* harc_amd_set_fastq_device for a BGZF-compressed FASTQ in device memory: the context holds the same inputs afterwards, byte for byte */
int harc_amd_set_fastq_bgzf_device(harc_amd_ctx *ctx, const uint8_t *d_bgzf, uint64_t n_bytes, uint64_t *n_records_out);
/* stage-II inputs when stage I ran elsewhere (the file family of reorder.cpp:722-830): host buffers.
   dna/dna_s are text with stride readlen+1 */
int harc_amd_set_stage1_streams(harc_amd_ctx *ctx, const char *temp_dna, const uint8_t *flag, const uint8_t *pos,
                                const uint32_t *order, const uint8_t *rc, uint32_t n_main,
                                const char *temp_dna_singleton, const uint32_t *order_singleton, uint32_t n_singleton);

/* ---- multi-GPU sharding helpers (BASELINE.json north_star: reads shard by k-mer bucket, one all-to-all, then every GPU
   runs the whole path on its shard).  Device buffers of params.device. */
/* 2-bit pack n ASCII reads into the caller's buffer of n*ceil(2*readlen/64) u64 (layout of harc_amd_set_reads_packed_device) */
int harc_amd_pack_reads_device(harc_amd_ctx *ctx, const char *d_ascii, uint32_t n_reads, uint32_t stride, uint64_t *d_packed_out);
/* bucket[i] = hash(canonical minimizer, k=15, of the whole read i) % n_buckets: reads that overlap by >= ~half a read
   share a minimizer with high probability and land on the same GPU */
int harc_amd_bucket_reads_device(harc_amd_ctx *ctx, const uint64_t *d_packed, uint32_t n_reads, uint32_t n_buckets, uint32_t *d_bucket_out);
/* the send buffer of the all-to-all in one call: reads grouped by bucket (bucket 0 first, original order inside a bucket) and the
   number of reads per bucket (n_buckets u64, device memory) */
int harc_amd_partition_reads_device(harc_amd_ctx *ctx, const uint64_t *d_packed, uint32_t n_reads, uint32_t n_buckets, uint64_t *d_packed_out, uint64_t *d_counts_out);

/* ---- multi-GPU run: one process (one context) per GPU, RCCL over xGMI.  The reference has no counterpart (its parallelism is OpenMP
   threads over one address space, reorder.cpp:455-457); what it fixes is the archive contract the merged result must meet: stream
   files read_*.txt.<shard> discovered by their count (harc:171, decoder.cpp:90-140), read_order.bin = original index of every
   decoded clean read in stream order, singletons last (decoder_preserve.cpp:246-290), read_order_N_pe.bin likewise for the reads
   with N (:212-244), read_order_N.bin = original record of every N read (merge_N.cpp:37-57).
   Bootstrap mirrors ncclGetUniqueId / ncclCommInitRank: rank 0 obtains an id, the caller ships the bytes to the other ranks (a
   file, MPI, torch.distributed, ...), every rank calls harc_amd_comm_init. */
#define HARC_AMD_COMM_ID_BYTES 128
int harc_amd_comm_get_id(uint8_t *id, size_t id_bytes);                                   /* id_bytes >= HARC_AMD_COMM_ID_BYTES */
int harc_amd_comm_init(harc_amd_ctx *ctx, const uint8_t *id, size_t id_bytes, int32_t world, int32_t rank);   /* ncclCommInitRank on params.device */
/* test transport: chunks travel through files of a shared directory, so that several ranks can share ONE GPU (RCCL refuses that) */
int harc_amd_comm_init_mailbox(harc_amd_ctx *ctx, const char *dir, int32_t world, int32_t rank);
int harc_amd_comm_barrier(harc_amd_ctx *ctx);
int harc_amd_comm_destroy(harc_amd_ctx *ctx);
/* The context holds this rank's slice of the job (harc_amd_set_reads_* / set_nreads_* / set_fastq_device).  Reads are bucketed by
   the hash of their canonical minimizer, grouped by destination and moved with ONE all-to-all(v) -- ncclGroupStart, ncclSend /
   ncclRecv per peer, ncclGroupEnd -- carrying 8W + 4 bytes per clean read (packed read + u32 global id) and 8 W3 + 4 per read with N.
   Afterwards harc_amd_reorder / harc_amd_encode work on the shard and HARC_AMD_S2_ORDER / HARC_AMD_S2_ORDER_N_PE hold GLOBAL ids
   (clean read i of rank r = sum of the clean reads of ranks < r, + i).  The slice itself stays with the context: calling the
   function again repeats the exchange.  info (8 u64, may be NULL): [0] clean reads of the whole job [1] reads with N [2] FASTQ
   records [3] this rank's first clean id [4] first N id [5] first record [6] clean reads received [7] N reads received. */
int harc_amd_shard_exchange(harc_amd_ctx *ctx, uint64_t *info);
/* Design (R): replicate the reads, partition the CHAINS.  One all-gather puts the reads of the whole job on every GPU in global id order;
   harc_amd_reorder then builds the whole index on every GPU, walks only the chains this rank owns and all-gathers the walked steps once per
   super-round; harc_amd_reorder / harc_amd_encode deliver, on EVERY rank, byte for byte what one GPU produces from the concatenated input
   (reorder.cpp:455-457 has one address space: this is its multi-GPU form that keeps the compression ratio; the bucket shard above trades
   ratio for memory and speed).  Every GPU must hold the whole job.  info as for harc_amd_shard_exchange. */
int harc_amd_replicate_exchange(harc_amd_ctx *ctx, uint64_t *info);
/* The stages read the context's own slice again (as before the first exchange); the results of the last run go, the communicator stays. */
int harc_amd_shard_reset(harc_amd_ctx *ctx);

/* ---- compute (all on params.device, asynchronous internally, synchronised before return) */
int harc_amd_reorder(harc_amd_ctx *ctx);      /* index build + chaining: reorder.cpp:277-703 */
int harc_amd_encode(harc_amd_ctx *ctx);       /* encoder.cpp:154-616 on the stage-I result held in HBM (or set_stage1_streams) */
int harc_amd_pack_order(harc_amd_ctx *ctx);   /* pack_order.cpp:20-77 on HARC_AMD_S2_ORDER */

/* ---- outputs */
int harc_amd_get_stream(harc_amd_ctx *ctx, int32_t stream_id, int32_t shard, const void **ptr, size_t *len);
int harc_amd_get_counters(harc_amd_ctx *ctx, harc_amd_counters *out);

/* ---- round-trip check at any size (decode side, decoder.cpp:90-169, restated on the GPU).
   Signature of a read multiset: sig[0] = number of reads, sig[1] = sum and sig[2] = xor of a 64-bit hash of every read
   (FNV-1a over the bases A0 C1 G2 T3 N4, then a 64-bit finaliser).  Order-independent, so the decoded output of any
   (num_chains, num_steps, num_thr) can be compared with the input reads without materialising either. */
int harc_amd_decode_signature(harc_amd_ctx *ctx, uint64_t sig[3]);         /* decodes the context's stage-II streams */
int harc_amd_reads_signature_device(harc_amd_ctx *ctx, const char *d_ascii, uint32_t n_reads, uint32_t stride, uint64_t sig[3]);
int harc_amd_input_signature(harc_amd_ctx *ctx, uint64_t sig[3]);           /* of the clean + N reads the context currently holds */

/* Digest of the stage-II streams of the last harc_amd_encode (needs params.stream_digest = 1), computed on the device from the very buffers the
   streams are copied out of: out[0] read_seq.txt.<e>(+.tail) of all shards and their cuts, out[1] read_noise / read_noisepos / read_pos and their
   cuts, out[2] read_rev.txt.<e>(+.tail), read_singleton.txt(+.tail), input_N.dna, out[3] read_order.bin and read_order_N_pe.bin.  Position-dependent
   64-bit sums: equal streams give equal words, a changed, moved, lost or added byte changes them (encoder.cpp:190-196,457-503 name the files). */
int harc_amd_stream_digest(harc_amd_ctx *ctx, uint64_t out[4]);
/* sha256 (hex) of the kernel sources this library was built from: ties a committed profile (profiles/k_steps_traffic.json) to a build */
const char *harc_amd_build_id(void);
/* 1 when this library was built with the named optional part: "test_transport" (the file-mailbox transport of the one-GPU multi-rank tests), "experiments" (schedule constants from the environment), "spack" (the packed stream file), "qmap" (lossy quality values); 0 otherwise */
int harc_amd_build_has(const char *feature);
/* Self-test of the library's launch geometry (one thread per item over n items through harc_gid / harc_gid32, and four lanes per item in folded workgroups, n beyond 2^32 included: a one-dimensional grid of 2^32 and more
 * work-items is cut short without an error on this platform).  *visited == n and *index_sum == n (n - 1) / 2 mod 2^64 when every item was visited once. */
int harc_amd_selftest_launch(harc_amd_ctx *ctx, uint64_t n, uint64_t *visited, uint64_t *index_sum);
/* Self-test of the index build: the very harc_dict_alloc + harc_dict_build the stages run, over n UNSCRAMBLED 64-bit keys in host memory with the ids
 * 0 .. n-1, into a slot array that holds a non-zero byte pattern beforehand (the build must not depend on cleared memory).  slots_per_read 2..4, 0 = the
 * library's choice; bigthresh as DictDev.bigthresh (0 = no SLOT_BIG); want_large != 0 lists the bins of more than 16 keys as (slot << 1) | 1.
 * slots == NULL: size query, *cap alone (with slots_per_read = 0 the library chooses by the memory free at that moment: a later call may choose another
 * cap, and then refuses a buffer that is too small).  Else *cap holds on entry how many 16-byte slots `slots` has room for (HARC_AMD_EINVAL when the table is larger),
 * and out come *cap, *nbins, slots[*cap] (key u64, start u32, count u32), ids[n], and -- with want_large -- large[min(*n_large, large_capacity)] and
 * *n_large.  Nothing stays allocated, and after an error return the context is as usable as before. */
int harc_amd_selftest_index(harc_amd_ctx *ctx, const uint64_t *keys, uint64_t n, int32_t slots_per_read, uint32_t bigthresh, int32_t want_large,
                            uint64_t *cap, uint32_t *nbins, void *slots, uint32_t *ids, uint64_t *large, uint64_t large_capacity, uint64_t *n_large);
/* Self-test of stage II's contig structure: the very code the encoder runs, over flag[n] ('0' = the read starts a contig) and pos[n] (the read's shift
 * against the read before it) in host memory, for reads of `readlen` bases, encoder shards of q reads and contigs cut every cut + 1 reads (the encoder:
 * 10 000 000).  Out come head[n], cid[n] (heads before the read), gstart[n] (first column), chead[*ncontigs] (the caller's buffer has room for n),
 * *ncontigs, *total (columns) and *fellback: 0 when the single scan did it, 1 when a read lay more than `cut` reads behind the last flag-'0' read or
 * shard start and the passes that cut contigs ran.  Nothing stays allocated. */
int harc_amd_selftest_contigs(harc_amd_ctx *ctx, const uint8_t *flag, const uint8_t *pos, uint64_t n, int32_t readlen, uint32_t q, uint32_t cut, uint8_t *head, uint32_t *cid,
                              uint64_t *gstart, uint32_t *chead, uint32_t *ncontigs, uint64_t *total, int32_t *fellback);
/* Self-test of the probe table's regular prefix (host code, no device): *nprobe = the probes of one chain step for these parameters (reorder.cpp:517-649:
 * shift by shift, forward then reverse, dictionary 0 then 1, a probe left out where its k-mer leaves the read), *nreg = how many leading shifts hold all
 * four of them in that order -- below it probe 4 j + 2 dir + dict is (shift j, dir, dict), which the dense chain kernel's carry relies on.  maxmatch <= 255. */
int harc_amd_selftest_probe_prefix(const harc_amd_params *p, int32_t *nprobe, int32_t *nreg);

/* Where the wall time of this process's last harc_amd_compress_fastq_files_ex went, in seconds (the end-to-end leg of bench.py; preprocess.cpp:81-121 + harc:50-69):
 * out[0] context + device pool, [1] ingest (file -> HBM -> packed stores; reads, uploads and kernels overlapped), [2] of it the calling thread waiting for
 * the file reader threads, [3] of it the device's line index / classify / pack passes, [4] reorder, [5] encode (the D2H of the streams inside),
 * [6] stream files written, [7] total up to there (the -q files of a run without -p come after it), [8] of [1] the BGZF member scan and inflate
 * (0 for a plain file).  n = how many of them the caller wants. */
int harc_amd_last_fastq_timing(double *out, int32_t n);

/* ---- file contract: drop-ins for the reference's stage programs.  basedir as argv[1] of those programs. */
int harc_amd_reorder_files(const harc_amd_params *params, const char *basedir);
int harc_amd_encoder_files(const harc_amd_params *params, const char *basedir);
int harc_amd_compress_files(const harc_amd_params *params, const char *basedir);
int harc_amd_pack_order_files(const harc_amd_params *params, const char *basedir);
/* harc:50-69 in one call: FASTQ file -> read_order_N.bin, numreads.bin and every stage-II file, parsed on the GPU, no
   input_clean.dna / temp.dna round trips */
int harc_amd_compress_fastq_files(const harc_amd_params *params, const char *fastq, const char *basedir);
/* the same with the reference's -p / -q switches (preprocess.out's 3rd and 4th argument, harc:50).  preserve_quality: also writes
   output/output.quality and output/output.id -- in file order with preserve_order (preprocess.cpp:64-69), otherwise gathered by the
   post-encoding orders exactly as reorder_quality.out does (reorder_quality.cpp:47-219, quirks included: see oracle/harc_oracle.c
   harc_oracle_quality).  preserve_order itself changes nothing else here: pack_order stays a separate call (harc:112).
   The file may be larger than HBM in every mode: it is ingested a piece at a time; without preserve_order the quality values and ids are
   then permuted by streaming the file again once per bin of output (reorder_quality.cpp:61-77 bins through host memory).
   The file may be BGZF (what bgzip writes; told by its first bytes): its members are inflated on the GPU, piece by piece, and every output file is
   the one the plain FASTQ with the same text gives.  Any other gzip is refused with HARC_AMD_EINVAL before a device is touched. */
int harc_amd_compress_fastq_files_ex(const harc_amd_params *params, const char *fastq, const char *basedir, int32_t preserve_order, int32_t preserve_quality);
/* The files of a -q run back into one FASTQ file: line i of dna_path (what the decoders write: fixed-length reads, one per line), of id_path and of
   quality_path become record i of out_path,  id \n read \n + \n quality \n  (harc_amd_fastq_assemble_device).  The read length is the length of the first
   line of dna_path (more than 255: HARC_AMD_EINVAL); only `device` is taken from params.  The output is size(id) + n * (2 * readlen + 4) bytes with
   n = size(dna) / (readlen + 1), known before a byte is read.  HARC_AMD_EINVAL before any GPU work: size(dna) is no multiple of readlen + 1, or
   size(quality) != size(dna).  The job runs in pieces of the id file (256 MiB of id text; HARC_AMD_FQOUT_PIECE=bytes in tests; a piece grows until it holds
   a whole line), so the files may be larger than device memory.  An id file whose line count differs from n: HARC_AMD_EINVAL naming both counts (the .id
   file the reference writes WITHOUT -p for an input with N reads can be a line short, and pairs ids wrongly on such inputs anyway: see README).  On any
   failure out_path is removed.  HARC_AMD_TRACE=1: one "[fastq_out]" line on stderr (bytes, pieces, seconds in the kernel / waiting for readers / writers). */
int harc_amd_fastq_assemble_files(const harc_amd_params *params, const char *dna_path, const char *id_path, const char *quality_path, const char *out_path);
/* harc_amd_fastq_assemble_files is this call with bgzf = 0.  bgzf = 1: out_path is the same FASTQ text as BGZF (harc_amd_bgzf_deflate_device: every assembled
   piece is deflated where it sits in device memory; one end-of-file marker ends the file) -- a .fastq.gz that harc_amd_compress_fastq_files, bgzip -d, gzip -d and
   samtools read.  The file is a function of the FASTQ text alone: members are cut at multiples of 65 280 bytes of the whole text, whatever the pieces
   (HARC_AMD_FQOUT_PIECE, HARC_AMD_FEED_SLICE).  Empty inputs give the 28-byte marker.  Refusals and the removal of out_path on failure are those of the plain
   call.  HARC_AMD_TRACE=1: the "[fastq_out]" line also names text bytes, compressed bytes, members, stored members and the seconds in the deflate kernels. */
int harc_amd_fastq_assemble_files_ex(const harc_amd_params *params, const char *dna_path, const char *id_path, const char *quality_path, const char *out_path, int32_t bgzf);
/* == `preprocess.out <fastq> <basedir> <preserve_order> <preserve_quality> <readlen>` (src/preprocess.cpp:22-137, harc:50),
   the N split only; host code, feeds the boundary */
int harc_amd_preprocess_files(const char *fastq, const char *basedir, int32_t readlen);
/* == `decoder.out <basedir> <num_thr> <num_thr_e>` (src/decoder.cpp:44-172, harc:188; non -p): reads the stage-II stream files of
   num_thr_e shards under <basedir>/output and writes output/output.dna, byte-identical to the reference decoder */
int harc_amd_decoder_files(const harc_amd_params *params, const char *basedir, int32_t num_thr_e);
/* == `unpack_order.out` + `decoder_preserve.out` + `merge_N.out` (harc:183-185, -p): needs read_order.bin(+.tail) as written by
   pack_order, read_order_N_pe.bin and read_order_N.bin; writes output/output.dna = the reads in their original FASTQ order.
   The order is restored in bins of output lines (params.decode_memory_gb, the reference's -m; capped by what fits in HBM): every bin
   decodes the streams again and keeps its own lines, so neither HBM nor host memory grows with the archive (the reference bins
   through host memory and a temporary file, decoder_preserve.cpp:246-290) */
int harc_amd_decoder_preserve_files(const harc_amd_params *params, const char *basedir, int32_t num_thr_e);
/* One rank of a multi-GPU `./harc -c -g <world>`: reads its slice of the FASTQ file (cut at record boundaries near rank/world of the
   file), joins the communicator named by comm_spec -- "rccl:<file>" (rank 0 writes the ncclUniqueId there, the others wait for it) or
   "mailbox:<dir>" (test transport) --, exchanges, compresses its shard and writes read_*.txt.<rank*num_thr + e> into
   <basedir>/output plus its part of the whole-job files under <basedir>/output/.shard/.  preserve_quality needs preserve_order
   (quality values and ids then stay in file order, preprocess.cpp:64-69).  The file must be plain FASTQ: gzip / BGZF input is refused with
   HARC_AMD_EINVAL before any device call (./harc -g expands it first); so for harc_amd_compress_fastq_replicated_files. */
int harc_amd_compress_fastq_shard_files(const harc_amd_params *params, const char *fastq, const char *basedir, int32_t preserve_order,
                                        int32_t preserve_quality, int32_t world, int32_t rank, const char *comm_spec);
/* After every rank has finished: the whole-job files of the archive (read_singleton.txt(+.tail), input_N.dna, read_order.bin,
   read_order_N_pe.bin, read_order_N.bin, numreads.bin, read_meta.txt, output.quality / output.id) from the parts under .shard/,
   laid out as encoder.cpp:457-503 writes them: aligned reads of all shards first, then the unaligned ones.  Host code. */
int harc_amd_merge_shard_files(const char *basedir, int32_t world);
/* One rank of `./harc -c -g N` in design-(R) mode (HARC_AMD_MG_MODE=replicate): as harc_amd_compress_fastq_shard_files, but the reads are
   all-gathered (harc_amd_replicate_exchange) and the chains partitioned; rank 0 writes the streams of the whole job -- byte for byte those
   of a single-GPU run, num_thr stream files -- the other ranks only their slice's parts; harc_amd_merge_shard_files finishes the archive. */
int harc_amd_compress_fastq_replicated_files(const harc_amd_params *params, const char *fastq, const char *basedir, int32_t preserve_order,
                                             int32_t preserve_quality, int32_t world, int32_t rank, const char *comm_spec);

/* ---- The packed quality file X.quality.hq (./harc -c -q -Q; the format is written down in README.md, "The packed quality file"): n lines of exactly readlen
   quality values and a newline -> a 32-byte header and blocks of reads_per_block lines, each stored or coded with order-1 static rANS in 256 strands that a
   workgroup codes independently.  readlen is 1..255 whatever the context's own read length is; reads_per_block 0 = the default max(256, 2^22 / readlen), and
   reads_per_block * readlen may not exceed 2^30.  The packed bytes depend on nothing but the text and reads_per_block. */
/* Host only: bytes that n_reads lines take at most, 32 + blocks * 5 + n_reads * readlen (every block stored). */
uint64_t harc_amd_qpack_bound(uint64_t n_reads, int32_t readlen, uint32_t reads_per_block);
/* d_text (device memory, n_reads * (readlen + 1) bytes, any alignment) -> the packed form at d_out (device memory, any alignment), *n_out bytes; no byte outside
   [d_out, d_out + *n_out) is written.  flags bit 0: the 32-byte file header in front of the blocks (without it: the blocks alone, for a caller that packs a file
   in pieces).  d_out == NULL: the size alone (the blocks are coded to learn it); else HARC_AMD_EINVAL naming both numbers when out_capacity is smaller.
   harc_amd_qpack_bound is always enough.  A byte at a (readlen + 1)-stride position that is no newline, or a newline anywhere else: HARC_AMD_EINVAL with the
   counts.  Any other byte outside 33..126 is kept: its block is stored.  HARC_AMD_TRACE=1: one "[qpack]" line on stderr. */
int harc_amd_qpack_device(harc_amd_ctx *ctx, const char *d_text, uint64_t n_reads, int32_t readlen, uint32_t reads_per_block, int32_t flags, uint8_t *d_out,
                          uint64_t out_capacity, uint64_t *n_out);
/* The packed form with its header, n_bytes in device memory -> its lines at d_text, *n_out = n * (readlen + 1) bytes, both numbers from the header.
   d_text == NULL: the size alone; a smaller out_capacity: HARC_AMD_EINVAL naming both numbers.  Everything read is validated before it is trusted: a wrong
   magic, a block prefix that leaves the bytes, a mode other than 0 or 1, a symbol count that is not the bitmap's, a row that sums to neither 0 nor 4096, strand
   lengths that do not sum to the payload, a strand that ends early, a context that never occurs, a strand that does not end in state 2^23 at its last byte:
   HARC_AMD_EINVAL naming the block and its byte offset, never an access out of bounds.  What was written to d_text by then is unspecified. */
int harc_amd_qunpack_device(harc_amd_ctx *ctx, const uint8_t *d_packed, uint64_t n_bytes, char *d_text, uint64_t out_capacity, uint64_t *n_out);
/* The same two calls in a row on the host, through the functions of harc_amd/csrc/qv_block.h that the kernels compile: they touch no device, and they are what the
   kernels are held to, byte for byte (tests). */
int harc_amd_qpack_host(const char *text, uint64_t n_reads, int32_t readlen, uint32_t reads_per_block, int32_t flags, uint8_t *out, uint64_t cap, uint64_t *n_out);
int harc_amd_qunpack_host(const uint8_t *packed, uint64_t n_bytes, char *text, uint64_t cap, uint64_t *n_out);
/* quality_path (what -c -q writes: fixed-length lines) -> out_path, packed on the GPU.  The read length is that of the first line (more than 255:
   HARC_AMD_EINVAL); the file size must be a multiple of readlen + 1 (checked before a device is touched); only `device` is taken from params.  The job runs in
   pieces of whole blocks (64 blocks; HARC_AMD_QPACK_PIECE=blocks, HARC_AMD_QPACK_BLOCK=reads per block in tests) through the pinned ring, so the file may be
   larger than device memory; the output is the same file whatever the piece, slice or thread settings.  On any failure out_path is removed.  HARC_AMD_TRACE=1:
   one "[qpack]" line on stderr (text bytes, packed bytes, blocks, stored blocks, pieces, seconds in the kernels / waiting for readers / for writers). */
int harc_amd_qpack_files(const harc_amd_params *params, const char *quality_path, const char *out_path);
/* packed_path -> the quality file at out_path, n * (readlen + 1) bytes known from the header before anything is decoded.  A short file, a wrong magic, a block
   prefix that leaves the file or any damaged block: HARC_AMD_EINVAL; a failed read: HARC_AMD_EIO.  On any failure out_path is removed. */
int harc_amd_qunpack_files(const harc_amd_params *params, const char *packed_path, const char *out_path);

/* ---- Lossy quality values (./harc -c -q -b SPEC; README.md, "-b and what it promises"): every quality value of a quality text -- n_reads lines of exactly
   readlen bytes and a newline, readlen in 1..255, as above -- is replaced by a coarser one.  A value is a byte v in 33..126, its Phred score q = v - 33.
   Newlines, and bytes outside 33..126, are never changed.  Every rule lives once in harc_amd/csrc/qm_block.h, for host and device.  The schemes:
     kind 1, a table: v -> table[v].  Valid when table[v] == v for every v outside 33..126 and table[v] lies in 33..126 for every v inside.
     kind 2, run smoothing with radius R (1..46): every line is cut, left to right, into blocks -- a block starts at the first byte not yet in one and takes the
             next byte while max - min over the block stays <= 2 R -- and every byte of a block becomes floor((min + max) / 2): no value moves by more than R.
   An invalid map is refused by every call with HARC_AMD_EINVAL, naming the first offending byte value. */
typedef struct harc_amd_qmap {
    int32_t kind;          /* 1: table, 2: run smoothing */
    int32_t radius;        /* kind 2: R */
    uint8_t table[256];    /* kind 1 */
} harc_amd_qmap;
/* What a mapping did, over the values 33..126 only.  A NULL pointer in a call: not computed (the kernels then do nothing for it). */
typedef struct harc_amd_qmap_stats {
    uint64_t values;       /* n_reads * readlen */
    uint64_t changed;      /* values that are not what they were */
    uint64_t sum_abs;      /* sum of |v' - v| */
    uint64_t sum_sq;       /* sum of (v' - v)^2 */
    uint32_t max_abs;
    uint32_t distinct_in;  /* distinct values before ... */
    uint32_t distinct_out; /* ... and after */
    uint32_t reserved;
} harc_amd_qmap_stats;
/* Host only: a spec string -> its map.  "ill8" (the eight levels of README.md), "bin:T:H:L" (q' = H when q >= T, else L; 1 <= T <= 93, 0 <= L <= H <= 93),
   "cap:M" (q' = min(q, M); 0 <= M <= 93), "pblock:R" (kind 2; 1 <= R <= 46).  Integers only.  Anything else -- an unknown name, a missing or surplus field, a
   number out of range, trailing characters -- is HARC_AMD_EINVAL, and the message names the spec and the field. */
int harc_amd_qmap_parse(const char *spec, harc_amd_qmap *out);
/* The serial line-by-line mapper of qm_block.h on the host: what the kernels are held to, byte for byte (tests).  out == text (in place) or disjoint from it.
   The (readlen + 1)-stride check of harc_amd_qpack_device applies, with the same message. */
int harc_amd_qmap_host(const char *text, uint64_t n_reads, int32_t readlen, const harc_amd_qmap *map, char *out, harc_amd_qmap_stats *stats);
/* The same on the GPU: d_text -> d_out, n_reads * (readlen + 1) bytes of device memory each, any alignment, and the two alignments may differ.  d_out == d_text
   exactly (in place) or disjoint from it: any other overlap is HARC_AMD_EINVAL.  No byte outside d_out's bytes is written, and no load leaves the 16-byte-aligned
   hull of d_text's.  A table runs as one streaming pass, run smoothing with a workgroup per 256 lines.  A text that fails the stride check is refused after the
   pass: values of d_out may then have been mapped.  HARC_AMD_TRACE=1: one "[qmap] device call" line on stderr with the kernel's milliseconds. */
int harc_amd_qmap_device(harc_amd_ctx *ctx, const char *d_text, uint64_t n_reads, int32_t readlen, const harc_amd_qmap *map, char *d_out, harc_amd_qmap_stats *stats);
/* quality_path -> out_path (a different file), mapped on the GPU; only `device` is taken from params.  The file runs through the pinned ring in pieces of whole
   lines (64 MiB; HARC_AMD_QMAP_PIECE=lines in tests), so it may be larger than device memory; the output is the same file whatever the piece, slice or thread
   settings (HARC_AMD_FEED_SLICE, HARC_AMD_FEED_THREADS).  On any failure out_path is removed. */
int harc_amd_qmap_files(const harc_amd_params *params, const char *quality_path, const char *out_path, const harc_amd_qmap *map, harc_amd_qmap_stats *stats);
/* harc_amd_qpack_files over the mapped text: every uploaded piece is mapped in place in device memory in front of the coder, the mapped text never reaches a
   file.  The packed file is that of harc_amd_qpack_files over the output of harc_amd_qmap_files.  map == NULL: harc_amd_qpack_files itself (stats is not touched).
   HARC_AMD_TRACE=1: with a map the "[qpack]" line also names the seconds in the map's kernels. */
int harc_amd_qpack_files_ex(const harc_amd_params *params, const char *quality_path, const char *out_path, const harc_amd_qmap *map, harc_amd_qmap_stats *stats);

/* ---- The packed id file X.id.hi (./harc -c -q -I; the format is written down in README.md, "The packed id file"): an id text -- lines of any length, empty
   ones too, every one ended by a newline (a last line without one: HARC_AMD_EINVAL) -> a 32-byte header and blocks of lines_per_block lines, each stored or
   coded: a line against the line in front of it, token by token, as events of a static rANS stream, in 256 strands of consecutive lines that a workgroup codes
   independently.  lines_per_block 0 = the default 2^18; the text of a block may not exceed 2^30 bytes (HARC_AMD_EINVAL naming the block).  The packed bytes
   depend on nothing but the text and lines_per_block. */
#define HARC_AMD_IDPACK_NO_HEADER 1
/* Host only: bytes that n_lines lines in text_bytes bytes take at most, 32 + blocks * 9 + text_bytes (every block stored). */
uint64_t harc_amd_idpack_bound(uint64_t text_bytes, uint64_t n_lines, uint32_t lines_per_block);
/* d_text (device memory, text_bytes bytes, any alignment) -> the packed form at d_out (device memory, any alignment), *n_out bytes; no byte outside
   [d_out, d_out + *n_out) is written and none outside the text is read.  flags: HARC_AMD_IDPACK_NO_HEADER writes the blocks alone, without the 32-byte file
   header (for a caller that packs a file in pieces).  d_out == NULL: the size alone (the blocks are coded to learn it); else HARC_AMD_EINVAL naming both numbers
   when out_capacity is smaller.  harc_amd_idpack_bound is always enough.  A byte outside 32..126 that is no newline is kept: its block is stored.
   HARC_AMD_TRACE=1: one "[idpack]" line on stderr. */
int harc_amd_idpack_device(harc_amd_ctx *ctx, const char *d_text, uint64_t text_bytes, uint32_t lines_per_block, int32_t flags, uint8_t *d_out, uint64_t out_capacity,
                           uint64_t *n_out);
/* The packed form with its header, n_bytes in device memory -> its text at d_text, *n_out bytes, the number from the header.  d_text == NULL: the size alone; a
   smaller out_capacity: HARC_AMD_EINVAL naming both numbers.  Everything read is validated before it is trusted (README lists the checks): HARC_AMD_EINVAL
   naming the block and its byte offset, never an access outside the packed form or the text.  What was written to d_text by then is unspecified. */
int harc_amd_idunpack_device(harc_amd_ctx *ctx, const uint8_t *d_packed, uint64_t n_bytes, char *d_text, uint64_t out_capacity, uint64_t *n_out);
/* The same two calls in a row on the host, through the functions of harc_amd/csrc/id_block.h that the kernels compile: they touch no device, and they are what the
   kernels are held to, byte for byte (tests). */
int harc_amd_idpack_host(const char *text, uint64_t text_bytes, uint32_t lines_per_block, int32_t flags, uint8_t *out, uint64_t cap, uint64_t *n_out);
int harc_amd_idunpack_host(const uint8_t *packed, uint64_t n_bytes, char *text, uint64_t cap, uint64_t *n_out);
/* id_path (what -c -q writes) -> out_path, packed on the GPU; only `device` is taken from params.  The text goes through the pinned ring in byte ranges; the whole
   blocks that have arrived are packed, at most HARC_AMD_IDPACK_PIECE blocks (8) and 256 MiB of text a kernel call (one block where a block alone is longer), and the rest is carried into the next range, so the file may be
   larger than device memory; the output is the same file whatever the piece, slice or thread settings.  HARC_AMD_IDPACK_BLOCK=lines per block (tests: it is
   recorded in the file and changes its bytes).  On any failure out_path is removed.  HARC_AMD_TRACE=1: one "[idpack]" line on stderr (text bytes, packed bytes,
   blocks, stored blocks, pieces, seconds in the kernels / waiting for readers / for writers). */
int harc_amd_idpack_files(const harc_amd_params *params, const char *id_path, const char *out_path);
/* packed_path -> the id file at out_path, its size known from the header before anything is decoded.  A short file, a wrong magic, a block prefix that leaves the
   file or any damaged block: HARC_AMD_EINVAL; a failed read: HARC_AMD_EIO.  On any failure out_path is removed. */
int harc_amd_idunpack_files(const harc_amd_params *params, const char *packed_path, const char *out_path);

/* ---- The packed stream file X.hs (./harc -c -S; the format is written down in README.md, "The packed stream file"): text_bytes bytes of any values -> a
   32-byte header and blocks of block_bytes text bytes, each stored or coded with static rANS in 256 strands of consecutive bytes that a workgroup codes
   independently: with one table (order 0) or with a table per previous byte (order 1), whichever payload is smallest, and with the CRC-32 of its text.
   block_bytes 0 = the default 2^22, at most 2^30.  The packed bytes depend on nothing but the text and block_bytes. */
/* Host only: bytes that text_bytes bytes take at most, 32 + text_bytes + 13 * blocks (every block stored). */
uint64_t harc_amd_spack_bound(uint64_t text_bytes, uint32_t block_bytes);
/* d_text (device memory, any alignment) -> the packed form at d_out (device memory, any alignment), *n_out bytes; no byte outside [d_out, d_out + *n_out) is
   written and none outside the text is read.  flags bit 0: the 32-byte file header in front of the blocks (without it: the blocks alone, for a caller that
   packs a file in pieces).  d_out == NULL: the size alone (the blocks are coded to learn it); else HARC_AMD_EINVAL naming both numbers when out_capacity is
   smaller.  harc_amd_spack_bound is always enough.  HARC_AMD_TRACE=1: one "[spack]" line on stderr. */
int harc_amd_spack_device(harc_amd_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, uint32_t block_bytes, int32_t flags, uint8_t *d_out, uint64_t out_capacity,
                          uint64_t *n_out);
/* The packed form with its header, n_bytes in device memory -> its text at d_text, *n_out bytes, the number from the header.  d_text == NULL: the size alone; a
   smaller out_capacity: HARC_AMD_EINVAL naming both numbers.  Everything read is validated before it is trusted (README lists the checks): HARC_AMD_EINVAL
   naming the block and its byte offset, never an access outside the packed form or the text.  What was written to d_text by then is unspecified. */
int harc_amd_sunpack_device(harc_amd_ctx *ctx, const uint8_t *d_packed, uint64_t n_bytes, uint8_t *d_text, uint64_t out_capacity, uint64_t *n_out);
/* The same two calls in a row on the host, through the functions of harc_amd/csrc/sv_block.h that the kernels compile: they touch no device, and they are what the
   kernels are held to, byte for byte (tests). */
int harc_amd_spack_host(const uint8_t *text, uint64_t text_bytes, uint32_t block_bytes, int32_t flags, uint8_t *out, uint64_t cap, uint64_t *n_out);
int harc_amd_sunpack_host(const uint8_t *packed, uint64_t n_bytes, uint8_t *text, uint64_t cap, uint64_t *n_out);
/* in_path (any file) -> out_path, packed on the GPU; only `device` is taken from params.  The job runs in pieces of whole blocks (64 blocks;
   HARC_AMD_SPACK_PIECE=blocks; HARC_AMD_SPACK_BLOCK=text bytes per block in tests: it is recorded in the file and changes its bytes) through the pinned ring, so
   the file may be larger than device memory; the output is the same file whatever the piece, slice or thread settings.  On any failure out_path is removed.
   HARC_AMD_TRACE=1: one "[spack]" line on stderr (text bytes, packed bytes, blocks of each mode, pieces, seconds in the kernels / waiting for readers / for
   writers). */
int harc_amd_spack_files(const harc_amd_params *params, const char *in_path, const char *out_path);
/* packed_path -> the file at out_path, its size known from the header before anything is decoded.  A short file, a wrong magic, a block prefix that leaves the
   file or any damaged block: HARC_AMD_EINVAL; a failed read: HARC_AMD_EIO.  On any failure out_path is removed. */
int harc_amd_sunpack_files(const harc_amd_params *params, const char *packed_path, const char *out_path);
/* The two file calls over n_files pairs of paths, one after the other on one side context (harc_amd_stage streams_pack / streams_unpack).  Every input is
   looked for before a device is touched; the first failure ends the call: its output is removed, the outputs in front of it and all inputs stay. */
int harc_amd_spack_file_list(const harc_amd_params *params, int32_t n_files, const char *const *in_paths, const char *const *out_paths);
int harc_amd_sunpack_file_list(const harc_amd_params *params, int32_t n_files, const char *const *packed_paths, const char *const *out_paths);

/* ---- Checked archives (./harc -c -V, -d, -v; README.md, "-V and what it promises").  The digest of a text of n bytes is T(text) = (n, newlines, D) with
   D = sum over the offsets o of mix64(((o + 1) << 8) | byte_o) mod 2^64 (harc_amd/csrc/check_block.h): a changed byte always changes D, any other change goes
   unnoticed with probability about 2^-64, and pieces that know their first offset add up to the digest of the whole.  Not cryptographic. */
/* The nbytes bytes at d_text (device memory, any alignment; no load leaves the 16-byte-aligned hull of the text), byte i at offset first_offset + i of the whole
   text: acc[0] += nbytes, acc[1] += newlines, acc[2] += their D terms.  nbytes may be 0.  HARC_AMD_TRACE=1: one "[check] device call" line on stderr. */
int harc_amd_text_digest_device(harc_amd_ctx *ctx, const void *d_text, uint64_t nbytes, uint64_t first_offset, uint64_t acc[3]);
/* The same sums over host memory, serially on the host: what the kernel is held to (tests).  Touches no device. */
int harc_amd_text_digest_host(const void *text, uint64_t nbytes, uint64_t first_offset, uint64_t acc[3]);
/* out = T of the file at path, sent through the pinned ring in pieces of 64 MiB; only `device` is taken from params.  The answer is the same whatever
   HARC_AMD_FEED_THREADS and HARC_AMD_FEED_SLICE are; an empty file gives (0, 0, 0) and touches no device.  HARC_AMD_TRACE=1: one "[check]" line on stderr. */
int harc_amd_text_digest_files(const harc_amd_params *params, const char *path, uint64_t out[3]);
/* out = T of the text "read_0\nread_1\n..." of the reads the context holds, in input record order: after harc_amd_set_fastq_device (or the file ingest) from the
   packed clean reads, the packed reads with N and the record numbers of the latter (HARC_AMD_IN_ORDER_N); after harc_amd_set_reads_* alone the clean reads in
   their order.  out[0] = records * (readlen + 1), out[1] = records. */
int harc_amd_input_order_digest(harc_amd_ctx *ctx, uint64_t out[3]);
/* dna_path (what the decoders write: fixed-length reads, one per line; the read length is that of the first line) read once through the pinned ring:
   sig = the multiset signature of its reads (harc_amd_reads_signature_device's definition), t = T of its text.  Only `device` is taken from params. */
int harc_amd_reads_check_files(const harc_amd_params *params, const char *dna_path, uint64_t sig[3], uint64_t t[3]);
/* harc_amd_compress_fastq_files_ex that also records and checks (check != 0; 0: that call itself): the multiset signature of the reads as ingested is taken before
   stage I, and with preserve_order the order digest; after stage II the streams are decoded once on the GPU (harc_amd_decode_signature) and must give the same
   signature -- otherwise HARC_AMD_EINTERNAL naming both triples, and no stream file is written.  <basedir>/output/read.check then holds "HARCV1", the line
   "reads <count> <sum> <xor>" and, with preserve_order, "order <bytes> <D>", every value as 16 lowercase hex digits. */
int harc_amd_compress_fastq_files_checked(const harc_amd_params *params, const char *fastq, const char *basedir, int32_t preserve_order, int32_t preserve_quality, int32_t check);

/* ---- Paired-end input (./harc -c R1 -2 R2 -p, ./harc -d -p -q; README.md, "-2 and what it promises").
   The mate rule.  Let a be id line i of file 1 and b id line i of file 2, without their newlines, the '@' included, any bytes.  A pair satisfies at most one of
     same    b == a
     slash   |a| = |b| >= 2, a ends in "/1", b is a with its last byte '2'
     space   |a| = |b|, a has a first space at s with s + 1 < |a|, a[s + 1] = '1', b is a with byte s + 1 set to '2'
   The rule of two files is the one that EVERY pair satisfies; no pair at all gives same; otherwise the rule is none.  By construction apply(A, rule) == B.
   A pair's flags: bit 0 same, bit 1 slash, bit 2 space; a rule as a number: */
#define HARC_AMD_IDMATE_NONE 0
#define HARC_AMD_IDMATE_SAME 1
#define HARC_AMD_IDMATE_SLASH 2
#define HARC_AMD_IDMATE_SPACE 3
/* *flags_and = the AND of the flags of all pairs of lines of the two id texts in device memory (any alignment; no load leaves the 8-byte-aligned hull of a text),
   7 when they hold no line; *n_pairs = the pairs.  Texts with different line counts or a last line without its newline: HARC_AMD_EINVAL naming both counts.
   HARC_AMD_TRACE=1: one "[idmate] device call" line on stderr with the rule kernel's time. */
int harc_amd_idmate_rule_device(harc_amd_ctx *ctx, const char *d_a, uint64_t a_bytes, const char *d_b, uint64_t b_bytes, uint64_t *n_pairs, uint32_t *flags_and);
/* The same over host memory, serially: what the kernel is held to (tests).  Touches no device. */
int harc_amd_idmate_rule_host(const char *a, uint64_t a_bytes, const char *b, uint64_t b_bytes, uint64_t *n_pairs, uint32_t *flags_and);
/* The rule that a flag word over n_pairs pairs stands for; its name ("none", "same", "slash", "space"; "?" for anything else); a name -> its number, or -1. */
int32_t harc_amd_idmate_rule_of(uint32_t flags_and, uint64_t n_pairs);
const char *harc_amd_idmate_rule_name(int32_t rule);
int32_t harc_amd_idmate_rule_parse(const char *name);
/* The rule of two id files, walked in lockstep through the pinned ring: a byte range of A and the next of B per turn, min(lines of A, lines of B) whole lines are
   compared, the rest of both is carried into the next turn.  HARC_AMD_IDMATE_PIECE: bytes per range (default 256 MiB; tests: pieces of a few lines); the answer
   does not depend on it.  Different line counts or a last line without its newline: HARC_AMD_EINVAL.  Only `device` is taken from params. */
int harc_amd_idmate_rule_files(const harc_amd_params *params, const char *path_a, const char *path_b, int32_t *rule, uint64_t *n_pairs);
/* File 2's ids from file 1's: the whole lines of the id text at d_ids (device memory, any alignment) are patched in place -- slash: the byte in front of each
   newline, space: the byte behind each line's first space, '1' -> '2'; same and none patch nothing.  *bad = the lines where the byte to replace is not '1' or
   does not exist (they stay as they are): a damaged id file, or another rule than the one recorded, is counted instead of assembled. */
int harc_amd_idmate_apply_device(harc_amd_ctx *ctx, char *d_ids, uint64_t id_bytes, int32_t rule, uint64_t *bad);
int harc_amd_idmate_apply_host(char *ids, uint64_t id_bytes, int32_t rule, uint64_t *bad);
/* harc_amd_compress_fastq_files_checked over TWO files as one job, the order always kept: the records of fastq1 followed by those of fastq2 -- the archive of
   `cat fastq1 fastq2` without the copy.  Each file is plain FASTQ or BGZF on its own.  Neither may end inside a 4-line record or without its last newline (the file
   is named), and both must hold the same number of records (both counts are named); *records_per_file (may be null) = that number.  With preserve_quality
   <basedir>/output/output.quality holds the quality lines of both files in order, output.id the ids of fastq1 and output.id2 those of fastq2.
   <basedir>/output/read.pair holds "HARCP1" and "records <n>" (decimal). */
int harc_amd_compress_fastq_pair_files(const harc_amd_params *params, const char *fastq1, const char *fastq2, const char *basedir, int32_t preserve_quality, int32_t check,
                                       uint64_t *records_per_file);
/* harc_amd_fastq_assemble_files_ex for a paired archive: records [0, n) of dna_path / quality_path -> out1_path, records [n, 2 n) -> out2_path, n = records_per_file.
   rule none: id_path holds 2 n lines, the second file continues where the first stopped.  Any other rule: id_path holds n lines, the first file's; the second
   file's are made from them on the GPU in front of the assembly (harc_amd_idmate_apply_device's patch and count).  Another line count: HARC_AMD_EINVAL naming the
   counts.  bgzf: each output is the BGZF file of its own text.  On any failure neither output file is left. */
int harc_amd_fastq_assemble_pair_files(const harc_amd_params *params, const char *dna_path, const char *id_path, const char *quality_path, const char *out1_path,
                                       const char *out2_path, uint64_t records_per_file, int32_t rule, int32_t bgzf);

/* ---- Range restore (./harc -d -r FIRST:LAST; README.md, "-r and what it promises").  Lines are counted from 0 in every call below.
   A text of nbytes bytes holds as many lines as newlines.  out[0] = the newlines of the nbytes bytes at d_text (device memory, any alignment; no load leaves
   the 16-byte-aligned hull of the text), out[1] = the byte offset at which line k starts: 0 for k = 0, else one past the k-th newline (nbytes itself when that
   newline is the last byte), UINT64_MAX when the text holds fewer than k newlines.  One streaming read that leaves a count per workgroup, the library's scan over
   the counts, and a second launch in which only the workgroup whose span holds the k-th newline looks for it; no atomics.  nbytes may be 0, and is at most
   2^32 - 1 (HARC_AMD_EINVAL beyond: harc_amd_line_range_files walks a longer text in pieces).  HARC_AMD_TRACE=1: one "[linesel] device call" line on stderr. */
int harc_amd_line_offset_device(harc_amd_ctx *ctx, const void *d_text, uint64_t nbytes, uint64_t k, uint64_t out[2]);
/* The same over host memory, serially: what the kernels are held to (tests).  Touches no device. */
int harc_amd_line_offset_host(const void *text, uint64_t nbytes, uint64_t k, uint64_t out[2]);
/* out = the byte range [begin, end) of lines first_line .. first_line + n_lines - 1 of the file at path.  The file goes through the pinned ring in pieces of
   HARC_AMD_LINESEL_PIECE bytes (default 256 MiB; tests: a few bytes), the newline count is carried from piece to piece, and nothing behind the piece that holds the
   end of the last line is looked at.  A file with fewer lines: HARC_AMD_EINVAL naming the lines wanted and the lines found.  Only `device` is taken from params;
   first_line = 0 and n_lines = 0 touch no device. */
int harc_amd_line_range_files(const harc_amd_params *params, const char *path, uint64_t first_line, uint64_t n_lines, uint64_t out[2]);
/* harc_amd_qunpack_files / harc_amd_idunpack_files for lines first_line .. first_line + n_lines - 1 alone (n_lines >= 1): the 32-byte header is read, the block
   prefixes are walked with pread up to the last block that holds one of the lines (a prefix that leaves the file: HARC_AMD_EINVAL naming the block), only the
   blocks that hold one of the lines are read and decoded -- every check of the block decoders stays in force for them --, the first and the last of them are
   cut in device memory (quality: by the stride readlen + 1; ids: where harc_amd_line_offset_device finds the line), and out_path holds exactly the wanted
   lines.  Blocks outside the range are NEITHER READ NOR CHECKED.  A range that passes the header's line count: HARC_AMD_EINVAL naming both.  One status line on
   stdout: the blocks decoded and the bytes of packed_path that were read.  On any failure out_path is removed. */
int harc_amd_qunpack_range_files(const harc_amd_params *params, const char *packed_path, const char *out_path, uint64_t first_line, uint64_t n_lines);
int harc_amd_idunpack_range_files(const harc_amd_params *params, const char *packed_path, const char *out_path, uint64_t first_line, uint64_t n_lines);
/* harc_amd_decoder_files / harc_amd_decoder_preserve_files that write only the lines of n_ranges (1 or 2) ranges [first[r], first[r] + count[r]) of what those
   calls write, one range after the other, into output/output.dna; every count is at least 1.  With the order restored the bins of output lines run over the
   ranges alone.  Without it every shard is still decoded (where the lines with N of a shard start is only known after decoding it) and only the parts of each
   segment inside a range are written.  Every consistency check of the whole decode stays in force.  A range past the total: HARC_AMD_EINVAL naming the total.
   n_ranges = 0 is the whole decode. */
int harc_amd_decoder_range_files(const harc_amd_params *params, const char *basedir, int32_t num_thr_e, int32_t n_ranges, const uint64_t *first, const uint64_t *count);
int harc_amd_decoder_preserve_range_files(const harc_amd_params *params, const char *basedir, int32_t num_thr_e, int32_t n_ranges, const uint64_t *first, const uint64_t *count);

/* ---- Selection by name (./harc -d -q -L NAMES; README.md, "-L and what it promises").  The name of a line (harc_amd/csrc/namekey.h, once for host and device;
   the line without its newline, any bytes): a leading '@' is skipped, the name runs up to the first space or tab or to the line's end, and a name of at least
   3 bytes that ends in "/1" or "/2" loses those two bytes, once.  An empty name never matches.  A last line without its newline counts as a line in both texts.
   out[0] = where the name of line[0 .. n) starts, out[1] = its length.  Touches no device. */
int harc_amd_name_key_host(const void *line, uint64_t n, uint64_t out[2]);
/* d_flags[i] = 1 when the name of line i of the id text is the name of a line of the list, else 0: one byte per id line, room for every line of the text.
   Both texts lie in device memory at any alignment; no load leaves their 16-byte hulls.  The list's names go into an open-addressing table (the smallest power
   of two >= 2 x list lines slots, at least 64; a slot holds the 64-bit hash of namekey.h and a list line; claimed with one 32-bit atomicCAS, linear probing,
   equal names told from equal hashes by their bytes; the hashes are filled in by a launch behind the claims), then k_name_probe streams the id text, eight
   lanes a line and eight bytes a lane and step, without atomics.  *n_lines = the id lines, *n_names = the distinct names of the list that are not empty,
   *n_found = those of them that at least one id line carries.  All outputs are functions of the two texts alone.  names_bytes: at most 2^30; id_bytes: at most
   2^32 - 1 (HARC_AMD_EINVAL beyond: harc_amd_select_files walks a longer text in pieces).  HARC_AMD_SELECT_HASH_BITS=b (1 .. 64, tests) keeps the low b bits of
   every hash, table and probe alike: the outputs do not change.  HARC_AMD_TRACE=1: one "[select] device call" line on stderr with the probe kernel's time. */
int harc_amd_select_flags_device(harc_amd_ctx *ctx, const void *d_names, uint64_t names_bytes, const void *d_ids, uint64_t id_bytes, uint8_t *d_flags,
                                 uint64_t *n_lines, uint64_t *n_names, uint64_t *n_found);
/* The same over host memory, serially: what the kernels are held to (tests).  Touches no device. */
int harc_amd_select_flags_host(const void *names, uint64_t names_bytes, const void *ids, uint64_t id_bytes, uint8_t *flags, uint64_t *n_lines, uint64_t *n_names,
                               uint64_t *n_found);
/* The lines of a text whose flag byte is not zero, one behind the other at d_out (device memory, any alignment, room for `capacity` bytes; nothing outside
   the result's bytes is written).  stride > 0: line i is bytes [i stride, (i + 1) stride) and nbytes = n_lines x stride (HARC_AMD_EINVAL otherwise); every lane
   owns 16 bytes of the output and writes them with one aligned store where the output allows.  stride 0: lines of any length, n_lines the text's lines
   (HARC_AMD_EINVAL naming both otherwise), each copied with its newline, a last line without one as it is.  nbytes at most 2^32 - 1.  The offsets come from the
   library's scan over the flags.  *out_bytes = the bytes of the result; more than capacity: HARC_AMD_EINVAL naming both, nothing written. */
int harc_amd_lines_gather_device(harc_amd_ctx *ctx, const void *d_text, uint64_t nbytes, uint64_t stride, const uint8_t *d_flags, uint64_t n_lines, void *d_out,
                                 uint64_t capacity, uint64_t *out_bytes);
/* The same over host memory, serially (tests).  Touches no device. */
int harc_amd_lines_gather_host(const void *text, uint64_t nbytes, uint64_t stride, const uint8_t *flags, uint64_t n_lines, void *out, uint64_t capacity, uint64_t *out_bytes);
/* The records of an archive's three texts whose id line carries a name of the list at names_path, in one call on one context: ids_path (lines of any length),
   dna_path and quality_path (lines of one length, the first line's of dna_path) -> out_ids_path, out_dna_path, out_quality_path, in their order.
   Phase A: the list is loaded whole, the id file walks through the pinned ring in pieces of HARC_AMD_SELECT_PIECE bytes (default 256 MiB; tests: a few bytes), what
   lies behind a piece's last whole line is carried, the probe runs on every piece's whole lines, the flags of the whole job stay resident at one byte a line.
   Phase B: each file goes through the ring in pieces of whole lines (the fixed-length files HARC_AMD_SELECT_LINES lines a piece), every piece is gathered and
   drained into an output file whose size is known from the selection.
   pair_records = 0: record i is selected when the name of id line i is listed; the id file holds as many lines as dna_path.  pair_records = n > 0, an archive of a
   pair (dna_path and quality_path hold 2 n lines, file 1's records first): with a pair_rule other than HARC_AMD_IDMATE_NONE the id file holds n lines, line i
   selects records i and n + i, and out_ids holds the selected lines once; with HARC_AMD_IDMATE_NONE it holds 2 n lines, pair i is selected when line i or line
   n + i is listed, and out_ids holds both halves' selected lines.  out_dna / out_quality hold the selected records of [0, n), then of [n, 2 n).
   stats = { distinct names, names found, records selected, records } (for a pair: of each file).  missing (may be null) receives up to ten listed names that
   no record carries, in list order, a newline behind each, zero-terminated, cut to missing_cap bytes.  Nothing selected is a success with stats[2] = 0 and three
   empty files.  HARC_AMD_EINVAL naming both counts, and no output file left, for: id lines that are not the reads' lines (for a pair with a rule: half of them), a
   quality file whose size is not the reads' file's, a pair_records that is not the id file's lines (under none: half of them), a list of more than 2^30 bytes or
   without a name.  Only `device` is taken from params. */
int harc_amd_select_files(const harc_amd_params *params, const char *names_path, const char *ids_path, const char *dna_path, const char *quality_path,
                          const char *out_ids_path, const char *out_dna_path, const char *out_quality_path, uint64_t pair_records, int32_t pair_rule,
                          uint64_t stats[4], char *missing, uint64_t missing_cap);

/* ---- Match by sequence (./harc -d -M MOTIFS [-e K]; README.md, "-M and what it promises").  The rule (harc_amd/csrc/motif.h, once for host and device):
   the list is split at '\n' (a last line without its newline counts); a line that is empty or begins with '>' is skipped; every other line is a motif of 1 to 255
   bytes from ACGTNacgtn, folded to upper case, whose bases that are not N number more than K; equal motifs count once; at most 1024 distinct motifs and 2^20
   bytes.  Motif p of m bases matches read r of L bases when, for q = p or its reverse complement and some offset 0 <= o <= L - m, at most K of the positions j
   with q[j] != 'N' have r[o + j] != q[j]; a read byte that is not one of A C G T equals no motif base.  0 <= K <= 8.
   *n_motifs = the distinct motifs of the list.  HARC_AMD_EINVAL with the reason, naming the line, for a list the rule refuses.  Touches no device. */
int harc_amd_motifs_check_host(const void *list, uint64_t list_bytes, uint32_t K, uint64_t *n_motifs);
/* flags[i] = 1 when some motif of the list matches line i of the n_lines lines of readlen + 1 bytes at dna (a read and its newline), else 0; hit (may be NULL, room
   for 1024 bytes) receives per distinct motif, in list order, 1 when it matches at least one line; *n_found = their number.  Plain C++ from the rule, with byte
   comparisons: what the kernel is held to (tests).  Touches no device. */
int harc_amd_motif_flags_host(const void *list, uint64_t list_bytes, uint32_t K, const void *dna, uint64_t n_lines, uint32_t readlen, uint8_t *flags, uint8_t *hit,
                              uint64_t *n_motifs, uint64_t *n_found);
/* The same on the GPU over resident reads: d_dna and d_flags are device memory at any alignment, list and hit host memory.  The list is parsed on the host and
   goes to the device as a table of entries, every motif and its reverse complement as bit planes; k_motif_match turns every line into the planes lo, hi and bad
   with aligned 16-byte loads that do not leave the 16-byte hull of the text, eight lanes a read, and counts mismatches with XOR and popcount.  No atomics; flags
   and hits are a function of the two texts and K alone.  HARC_AMD_TRACE=1: one "[match] device call" line on stderr with the kernel's time. */
int harc_amd_motif_flags_device(harc_amd_ctx *ctx, const void *list, uint64_t list_bytes, uint32_t K, const void *d_dna, uint64_t n_lines, uint32_t readlen,
                                uint8_t *d_flags, uint8_t *hit, uint64_t *n_motifs, uint64_t *n_found);
/* The lines of dna_path (lines of one length, the first line's) whose read matches a motif of the list at motifs_path -> out_dna_path, in their order, in one call
   on one context.  ids_path and quality_path, both or neither (NULL): the lines of the same records of those texts -> out_ids_path, out_quality_path.
   Phase A: the table is loaded, dna_path walks through the pinned ring in pieces of HARC_AMD_MATCH_LINES whole lines (default 256 MiB worth; tests: a few), the
   flags of the whole job stay resident at one byte a line.  Phase B is the gather of harc_amd_select_files (HARC_AMD_SELECT_PIECE, HARC_AMD_SELECT_LINES).
   pair_records = n > 0 (only with the id and quality files): dna_path and quality_path hold 2 n lines, pair i is selected when read i or read n + i matches, and
   the layouts of the id file under pair_rule are those of harc_amd_select_files.
   stats = { distinct motifs, motifs found, records selected, records } (for a pair: of each file; without the side files: lines).  missing (may be NULL) receives up
   to ten motifs that no read matches, in list order, a newline behind each, zero-terminated, cut to missing_cap bytes.  Nothing selected is a success with
   stats[2] = 0 and empty files.  HARC_AMD_EINVAL / HARC_AMD_EIO with the reason, and no output file left, for a list the rule refuses, files that do not fit each
   other, or a file that cannot be read.  Only `device` is taken from params. */
int harc_amd_match_files(const harc_amd_params *params, const char *motifs_path, uint32_t K, const char *dna_path, const char *ids_path, const char *quality_path,
                         const char *out_dna_path, const char *out_ids_path, const char *out_quality_path, uint64_t pair_records, int32_t pair_rule,
                         uint64_t stats[4], char *missing, uint64_t missing_cap);

/* ---- The recovery record (./harc -c -P PCT writes X.hr, ./harc -R repairs from it; README: "-P and what it promises", "The recovery record (X.hr)").  Files are cut
   into blocks of B bytes, blocks into spans, spans into interleaved groups of at most 128 members; a group of k members gets m = min(128, max(1, ceil(k PCT / 100)))
   recovery blocks, recovery block i = XOR_j inverse(i ^ (128 + j)) * member_j over GF(2^8) with the polynomial 0x11D (a Cauchy matrix: any e <= m lost members of a
   group are rebuilt from any e intact recovery blocks).  harc_amd/csrc/gf_block.h holds the arithmetic, the geometry and the head of the record, once for host and device. */
/* out[b] = the digest of block b of n_blocks blocks of block_bytes bytes that lie one behind the other at d_data (device memory, 16-byte aligned): D of the text
   digest above with offsets counted from 0 inside the block, over block_bytes bytes, of the last block over last_bytes (1 .. block_bytes).  block_bytes: a multiple
   of 16 from 16 to 2^24.  One launch, a workgroup per block, no atomics; out is host memory.  No load leaves the 16-byte hull of the bytes digested. */
int harc_amd_block_digests_device(harc_amd_ctx *ctx, const void *d_data, uint64_t n_blocks, uint32_t block_bytes, uint32_t last_bytes, uint64_t *out);
int harc_amd_block_digests_host(const void *data, uint64_t n_blocks, uint32_t block_bytes, uint32_t last_bytes, uint64_t *out);
/* out[q] = XOR over s of coef[q * ns + s] * src[s], byte by byte over block_bytes bytes, for q < e (1 .. 128) outputs and s < ns (1 .. 256) sources.  d_src and
   d_out are host arrays of device pointers, each 16-byte aligned and naming block_bytes bytes; an output may not overlap a source.  coef is host memory.  The one
   kernel serves both directions: making the record (sources a group's members, coef the Cauchy rows) and repairing (sources the intact members and recovery
   blocks, coef the solved matrix).  HARC_AMD_TRACE=1: one "[recovery] device call" line on stderr. */
int harc_amd_gf_combine_device(harc_amd_ctx *ctx, uint32_t block_bytes, int32_t ns, const void *const *d_src, int32_t e, void *const *d_out, const uint8_t *coef);
/* The same over host memory (any alignment), on the packed words of gf_block.h: what the kernel is held to (tests).  Touches no device. */
int harc_amd_gf_combine_host(uint32_t block_bytes, int32_t ns, const void *const *src, int32_t e, void *const *out, const uint8_t *coef);
/* out_path = the recovery record over the n_files files at paths (their base names are recorded and must differ), pct 1 .. 100.  Every file goes through the pinned
   ring a span at a time: block digests, the file's D, one combine launch for the groups of the span, the recovery blocks written into the record.  The geometry is
   HARC_AMD_RECOVERY_BLOCK (bytes, default 65536), HARC_AMD_RECOVERY_SPAN (blocks, default 8192) and HARC_AMD_RECOVERY_GROUP (blocks, default and maximum 128); it is
   recorded in the file.  The record's bytes do not depend on HARC_AMD_FEED_SLICE or HARC_AMD_FEED_THREADS.  stats (may be NULL): files, bytes protected, bytes of
   the record, data blocks, groups.  On any failure out_path is removed.  Only `device` is taken from params. */
int harc_amd_recovery_make_files(const harc_amd_params *params, int32_t n_files, const char *const *paths, uint32_t pct, const char *out_path, uint64_t *stats);
/* The files that the record at record_path names, looked for in the record's own directory, held against it: every block of every file and every recovery block
   is digested on the GPU and compared on the host.  check writes nothing; repair rebuilds the lost blocks of every group that holds at least as many intact recovery
   blocks (each rebuilt block is digested and compared with its recorded digest before a byte is written; then the file is synced and its D compared), extends a
   file that is shorter than recorded and creates one that is missing.  A file with a group that cannot be solved is not touched; the other files still are.
   report (may be NULL) receives the lines "[recovery] <name> ok | repaired: x of nb blocks | damaged: x of nb blocks, recoverable | NOT recoverable: span s group g
   has lost e of k blocks and holds x recovery blocks", one per file, in front of them what is wrong with the record itself, cut to report_capacity.
   *status = 0 when every file verifies in the end (check: when nothing at all is damaged, the record included), else 1.  A record whose two head copies both fail,
   a head whose counts do not give the record's size, a name with a '/', a file longer than recorded: HARC_AMD_EINVAL, and nothing is written.  No record:
   HARC_AMD_EIO. */
int harc_amd_recovery_check_files(const harc_amd_params *params, const char *record_path, char *report, uint64_t report_capacity, int32_t *status);
int harc_amd_recovery_repair_files(const harc_amd_params *params, const char *record_path, char *report, uint64_t report_capacity, int32_t *status);
/* The same two jobs in plain C++ on the host, through the functions of gf_block.h: they touch no device, and they are what the kernels and the file calls are held
   to (tests).  block_bytes, span_blocks, group_blocks: 0 = the environment's or the default.  write = 0: check, else repair. */
int harc_amd_recovery_make_host(int32_t n_files, const char *const *paths, uint32_t pct, uint32_t block_bytes, uint32_t span_blocks, uint32_t group_blocks, const char *out_path, uint64_t *stats);
int harc_amd_recovery_repair_host(const char *record_path, int32_t write, char *report, uint64_t report_capacity, int32_t *status);

/* ---- Third lines (./harc -c -q, ./harc -d -q; README.md, "Third lines and what is promised").
   The rule.  Let a be the id line of a record and t its third line, without their newlines, any bytes (a '\r' is a byte like any other).  A record satisfies
     bare    |t| = 1 and t[0] = '+'
     same    |t| = |a| >= 1, t[0] = '+' and t[1..] = a[1..] byte for byte (a[0] is not looked at)
   (a = "@" with t = "+" satisfies both).  The rule of a job is the one that EVERY record satisfies: no record gives bare, the bare bit left standing gives bare,
   otherwise the same bit gives same, otherwise the third lines are dropped (mixed files are).  A record takes part when its third line is there: a last record
   cut short behind its first or second line does not.  A record's flags: bit 0 bare, bit 1 same; a rule as a number: */
#define HARC_AMD_THIRD_DROPPED 0
#define HARC_AMD_THIRD_BARE 1
#define HARC_AMD_THIRD_SAME 2
/* *flags_and = the AND of the flags of all records of the FASTQ text in device memory (any alignment; no load leaves the 8-byte-aligned hull of the text), 3 when
   no record takes part; *n_records = the records that did.  The call builds its own line index; a third line of length 1 is decided from the index and its one
   byte, so a text with bare third lines has no id byte read.  harc_amd_compress_fastq_files_ex and its kin run the same kernel over every piece of the ingest
   when preserve_quality is set and write <basedir>/output/read.third ("HARCT1", then "third same" or "third dropped") unless the rule is bare.
   HARC_AMD_TRACE=1: one "[third] device call" line on stderr with the rule kernel's time. */
int harc_amd_third_rule_device(harc_amd_ctx *ctx, const char *d_fastq, uint64_t n_bytes, uint64_t *n_records, uint32_t *flags_and);
/* The same over host memory, serially: what the kernel is held to (tests).  Touches no device. */
int harc_amd_third_rule_host(const char *fastq, uint64_t n_bytes, uint64_t *n_records, uint32_t *flags_and);
/* The rule that a flag word over n_records records stands for; its name ("dropped", "bare", "same"; "?" for anything else); a name -> its number, or -1. */
int32_t harc_amd_third_rule_of(uint32_t flags_and, uint64_t n_records);
const char *harc_amd_third_rule_name(int32_t rule);
int32_t harc_amd_third_rule_parse(const char *name);
/* harc_amd_fastq_assemble_device, harc_amd_fastq_assemble_files_ex and harc_amd_fastq_assemble_pair_files with the rule of the third lines; those calls are these
   with HARC_AMD_THIRD_BARE.  HARC_AMD_THIRD_SAME: record i is  id_i \n read_i \n '+' id_i[1..] \n quality_i \n, the output holds 2 * size(id) + n * (2 * readlen + 2)
   bytes (still known before a byte is read), and in a pair the second file's third lines carry the second file's ids.  An id line of length 0 cannot be repeated
   behind a '+': such lines are counted on the device, the call fails with HARC_AMD_EINVAL naming the count and out_path is removed.  HARC_AMD_THIRD_DROPPED writes
   what bare writes.  Any other number: HARC_AMD_EINVAL. */
int harc_amd_fastq_assemble_third_device(harc_amd_ctx *ctx, const char *d_ids, uint64_t id_bytes, const char *d_dna, const char *d_quality, uint32_t n_records,
                                         int32_t readlen, char *d_out, uint64_t out_capacity, uint64_t *n_out, int32_t third);
int harc_amd_fastq_assemble_third_files(const harc_amd_params *params, const char *dna_path, const char *id_path, const char *quality_path, const char *out_path,
                                        int32_t bgzf, int32_t third);
int harc_amd_fastq_assemble_third_pair_files(const harc_amd_params *params, const char *dna_path, const char *id_path, const char *quality_path, const char *out1_path,
                                             const char *out2_path, uint64_t records_per_file, int32_t rule, int32_t bgzf, int32_t third);

#ifdef __cplusplus
}
#endif
#endif /* HARC_AMD_H */
