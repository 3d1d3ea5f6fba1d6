// main.cpp -- harc_amd_stage: command-line twin of the reference's stage executables.  The table `commands` below names every command with its words; the ones
// that stand for a line of the reference's driver are
//   reorder  <basedir> <readlen> [num_thr] [num_chains] [num_steps]        == src/reorder.out  <basedir>   (harc:67)
//   encoder  <basedir> <readlen> [num_thr] [num_chains] [num_steps]        == src/encoder.out  <basedir>   (harc:69)
//   compress <basedir> <readlen> [num_thr] [num_chains] [num_steps]        == both, stage I -> II handed over in HBM
//   pack_order <basedir> <readlen>                                         == src/pack_order.out <basedir> (harc:112)
//   decoder <basedir> <readlen ignored> <num_thr_e>                        == src/decoder.out <basedir> <num_thr> <num_thr_e> (harc:188)
//   decoder_preserve <basedir> <ignored> <num_thr_e> [memory_gb]           == unpack_order + decoder_preserve + merge_N (harc:174-185, -m = MAX_BIN_SIZE)
//   preprocess <basedir> <readlen> <fastq>                                 == src/preprocess.out <fastq> <basedir> .. <readlen> (harc:50)
//   compressfq <basedir> <readlen> <fastq> [num_thr] [num_chains] [num_steps] [preserve_order] [preserve_quality] [check]
//                                                                          == preprocess + reorder + encoder (+ reorder_quality), FASTQ parsed on the GPU
// readlen / num_thr arrive as arguments instead of the compile-time macros of src/config.h (harc:52-63).
// (every <first> counts lines from 0; ./harc -r counts from 1)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/harc_amd.h"

typedef unsigned long long ull;

// what a handler answers besides the library's code
enum {
    NEEDS = 1 << 20,    // the words are not the command's: main prints its "needs" line, status 2
    REFUSED,            // one word is not what it must be and the handler has said which: status 2
    DAMAGED             // the library's call went well and its report says that not every file verifies: status 1
};

// a decimal number that fits 64 bits and nothing else
static bool number(const char *s, uint64_t *v)
{
    char *end = nullptr;
    if (!*s || *s == '-' || *s == '+') return false;
    *v = strtoull(s, &end, 10);
    return *end == 0;
}

// [num_thr] [num_chains] [num_steps] from argv[at] on, as far as they are given
static void schedule_words(harc_amd_params *P, int argc, char **argv, int at)
{
    if (argc > at) P->num_thr = atoi(argv[at]);
    if (argc > at + 1) P->num_chains = atoi(argv[at + 1]);
    if (argc > at + 2) P->num_steps = atoi(argv[at + 2]);
}

// what a mapping of quality values did, one line on stdout
static void print_qmap(const char *spec, const harc_amd_qmap_stats *st)
{
    printf("[qmap] %s: %llu values, %llu changed, mean absolute change %.3f, max change %u, distinct values %u -> %u\n", spec, (ull)st->values,
           (ull)st->changed, st->values ? (double)st->sum_abs / (double)st->values : 0.0, st->max_abs, st->distinct_in, st->distinct_out);
}

// the spec of a mapping of quality values, or the library's reason on stderr
static bool qmap_word(const char *spec, harc_amd_qmap *M)
{
    if (harc_amd_qmap_parse(spec, M) == 0) return true;
    fprintf(stderr, "%s\n", harc_amd_last_error());
    return false;
}

// the optional words behind the fixed arguments of fastq_out and fastq_out_pair: [bgzf] [third], in that order and nothing else
static bool trailing_words(int argc, char **argv, int at, const char *behind, int *bgzf, int *third)
{
    *bgzf = *third = 0;
    if (at < argc && !strcmp(argv[at], "bgzf")) { *bgzf = 1; at++; }
    if (at < argc && !strcmp(argv[at], "third")) { *third = 1; at++; }
    if (at != argc) fprintf(stderr, "%s: behind %s only 'bgzf', 'third' or 'bgzf third' can follow (got '%s')\n", argv[1], behind, argv[argc - 1]);
    return at == argc;
}

// compressfq and compressfq_pair: the word behind <preserve_quality>, if there is one
static bool check_word(int argc, char **argv)
{
    if (argc > 10 && strcmp(argv[10], "check")) { fprintf(stderr, "%s: the argument behind <preserve_quality> can only be 'check' (got '%s')\n", argv[1], argv[10]); return false; }
    return true;
}

static int do_quality_spec(int argc, char **argv, harc_amd_params *)                // no device is touched
{
    harc_amd_qmap M;
    if (argc != 3) return NEEDS;
    return qmap_word(argv[2], &M) ? 0 : REFUSED;
}

static int do_digest(int, char **argv, harc_amd_params *P)                          // text_digest, reads_check
{
    uint64_t sig[3] = { 0, 0, 0 }, t[3] = { 0, 0, 0 };
    const bool reads = !strcmp(argv[1], "reads_check");
    const int rc = reads ? harc_amd_reads_check_files(P, argv[2], sig, t) : harc_amd_text_digest_files(P, argv[2], t);
    if (rc != 0) return rc;
    if (reads) printf("%016llx %016llx %016llx ", (ull)sig[0], (ull)sig[1], (ull)sig[2]);
    printf("%016llx %016llx %016llx\n", (ull)t[0], (ull)t[1], (ull)t[2]);
    return 0;
}

static int do_id_mates(int, char **argv, harc_amd_params *P)
{
    int32_t rule = 0; uint64_t pairs = 0;
    const int rc = harc_amd_idmate_rule_files(P, argv[2], argv[3], &rule, &pairs);
    if (rc == 0) printf("%s %llu\n", harc_amd_idmate_rule_name(rule), (ull)pairs);
    return rc;
}

static int do_recovery_make(int argc, char **argv, harc_amd_params *P)
{
    char *end = nullptr;
    const long pct = strtol(argv[2], &end, 10);
    if (!*argv[2] || *end || pct < 1 || pct > 100) return NEEDS;
    uint64_t st[5] = { 0, 0, 0, 0, 0 };
    const int rc = harc_amd_recovery_make_files(P, argc - 5, (const char *const *)(argv + 5), (uint32_t)pct, argv[4], st);
    if (rc == 0) printf("[recovery] %llu files, %llu bytes protected, %llu bytes of %s, %llu blocks, %llu groups\n", (ull)st[0], (ull)st[1], (ull)st[2], argv[4], (ull)st[3], (ull)st[4]);
    return rc;
}

static int do_recovery(int, char **argv, harc_amd_params *P)                        // recovery_check, recovery_repair: the report first, whatever the call answers
{
    static char report[1 << 16];
    int32_t status = 1;
    report[0] = 0;
    const int rc = !strcmp(argv[1], "recovery_check") ? harc_amd_recovery_check_files(P, argv[2], report, sizeof report, &status)
                                                      : harc_amd_recovery_repair_files(P, argv[2], report, sizeof report, &status);
    fputs(report, stdout);
    return rc != 0 ? rc : status ? DAMAGED : 0;
}

static int do_merge_shards(int, char **argv, harc_amd_params *) { return harc_amd_merge_shard_files(argv[2], atoi(argv[3])); }

static int do_fastq_out(int argc, char **argv, harc_amd_params *P)                  // the read length is the first line's of <dna>
{
    int bgzf = 0, third = 0;
    if (!trailing_words(argc, argv, 7, "<out>", &bgzf, &third)) return REFUSED;
    return third ? harc_amd_fastq_assemble_third_files(P, argv[2], argv[4], argv[5], argv[6], bgzf, HARC_AMD_THIRD_SAME)
           : bgzf ? harc_amd_fastq_assemble_files_ex(P, argv[2], argv[4], argv[5], argv[6], 1) : harc_amd_fastq_assemble_files(P, argv[2], argv[4], argv[5], argv[6]);
}

static int do_fastq_out_pair(int argc, char **argv, harc_amd_params *P)
{
    int bgzf = 0, third = 0;
    if (!trailing_words(argc, argv, 10, "<rule>", &bgzf, &third)) return REFUSED;
    char *end = nullptr;
    const ull records = strtoull(argv[8], &end, 10);
    if (!*argv[8] || *end) { fprintf(stderr, "fastq_out_pair: <records> must be a decimal number (got '%s')\n", argv[8]); return REFUSED; }
    const int32_t rule = harc_amd_idmate_rule_parse(argv[9]);
    if (rule < 0) { fprintf(stderr, "fastq_out_pair: <rule> must be none, same, slash or space (got '%s')\n", argv[9]); return REFUSED; }
    return third ? harc_amd_fastq_assemble_third_pair_files(P, argv[2], argv[4], argv[5], argv[6], argv[7], records, rule, bgzf, HARC_AMD_THIRD_SAME)
                 : harc_amd_fastq_assemble_pair_files(P, argv[2], argv[4], argv[5], argv[6], argv[7], records, rule, bgzf);
}

static int do_quality_map(int argc, char **argv, harc_amd_params *P)                // quality_map, and quality_pack (the read length is in the file)
{
    const bool pack = !strcmp(argv[1], "quality_pack");
    if (pack && argc <= 5) return harc_amd_qpack_files(P, argv[2], argv[4]);
    harc_amd_qmap M; harc_amd_qmap_stats ST;                                          // (quality_pack: the values mapped in front of the coder)
    if (!qmap_word(argv[5], &M)) return REFUSED;
    const int rc = pack ? harc_amd_qpack_files_ex(P, argv[2], argv[4], &M, &ST) : harc_amd_qmap_files(P, argv[2], argv[4], &M, &ST);
    if (rc == 0) print_qmap(argv[5], &ST);
    return rc;
}

static int do_quality_unpack(int, char **argv, harc_amd_params *P) { return harc_amd_qunpack_files(P, argv[2], argv[4]); }
static int do_id_pack(int, char **argv, harc_amd_params *P) { return harc_amd_idpack_files(P, argv[2], argv[4]); }
static int do_id_unpack(int, char **argv, harc_amd_params *P) { return harc_amd_idunpack_files(P, argv[2], argv[4]); }

static int do_gunzip(int, char **argv, harc_amd_params *P)
{
    harc_amd_gunzip_stats GS;
    const int rc = harc_amd_gunzip_files(P, argv[2], argv[4], &GS);
    if (rc == 0) printf("[gunzip] %llu members, %llu chunks, %llu starts found, %llu dropped, %llu repaired, %llu bytes of text\n", (ull)GS.members, (ull)GS.chunks,
                        (ull)GS.starts_found, (ull)GS.starts_dropped, (ull)GS.repair_walks, (ull)GS.text_bytes);
    return rc;
}

static int do_streams(int argc, char **argv, harc_amd_params *P)                    // streams_pack, streams_unpack
{
    if ((argc - 3) % 2) return NEEDS;
    const int np = (argc - 3) / 2;
    const char **in = (const char **)malloc(sizeof(char *) * 2 * (size_t)np), **out = in + np;
    if (!in) return HARC_AMD_ENOMEM;
    for (int k = 0; k < np; k++) { in[k] = argv[3 + 2 * k]; out[k] = argv[4 + 2 * k]; }
    const int rc = !strcmp(argv[1], "streams_pack") ? harc_amd_spack_file_list(P, np, in, out) : harc_amd_sunpack_file_list(P, np, in, out);
    free(in);
    return rc;
}

static int do_line_range(int, char **argv, harc_amd_params *P)
{
    uint64_t first = 0, count = 0, r[2] = { 0, 0 };
    if (!number(argv[3], &first) || !number(argv[4], &count)) return NEEDS;
    const int rc = harc_amd_line_range_files(P, argv[2], first, count, r);
    if (rc == 0) printf("%llu %llu\n", (ull)r[0], (ull)r[1]);
    return rc;
}

static int do_records_select(int argc, char **argv, harc_amd_params *P)
{
    uint64_t records = 0, st[4] = { 0, 0, 0, 0 }; int32_t rule = 0;
    static char missing[1 << 16];
    if (argc != 10 && argc != 13) return NEEDS;
    if (argc == 13) {
        if (strcmp(argv[10], "pair") || !number(argv[11], &records) || records < 1) return NEEDS;
        if ((rule = harc_amd_idmate_rule_parse(argv[12])) < 0) return NEEDS;
    }
    const int rc = harc_amd_select_files(P, argv[2], argv[4], argv[5], argv[6], argv[7], argv[8], argv[9], records, rule, st, missing, sizeof missing);
    if (rc != 0) return rc;
    printf("[select] %llu names, %llu found, %llu of %llu records\n", (ull)st[0], (ull)st[1], (ull)st[2], (ull)st[3]);
    for (const char *p = missing; *p;) { const char *e = strchr(p, '\n'); if (!e) break; printf("[select] not found: %.*s\n", (int)(e - p), p); p = e + 1; }
    return 0;
}

static int do_motifs_check(int argc, char **argv, harc_amd_params *)                // no device is touched
{
    uint64_t K = 0, n = 0;
    if (argc != 4 || !number(argv[3], &K) || K > 8) return NEEDS;
    FILE *f = fopen(argv[2], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return REFUSED; }
    static char list[(1 << 20) + 1];
    const size_t got = fread(list, 1, sizeof list, f);
    fclose(f);
    if (got > (size_t)1 << 20) { fprintf(stderr, "the list holds more than the 1048576 bytes of a list of motifs\n"); return REFUSED; }
    if (harc_amd_motifs_check_host(list, got, (uint32_t)K, &n) != 0) {
        const char *why = harc_amd_last_error(), *cut = strstr(why, ": ");      // (behind the call's own name)
        fprintf(stderr, "%s\n", cut ? cut + 2 : why);
        return REFUSED;
    }
    printf("%llu motifs\n", (ull)n);
    return 0;
}

static int do_records_match(int argc, char **argv, harc_amd_params *P)
{
    uint64_t K = 0, records = 0, st[4] = { 0, 0, 0, 0 }; int32_t rule = 0;
    static char missing[1 << 12];
    const char *ids = nullptr, *quality = nullptr, *out_ids = nullptr, *out_quality = nullptr;
    int at = 7;
    if (!number(argv[4], &K) || K > 8) return NEEDS;
    if (at < argc && !strcmp(argv[at], "q")) {
        if (argc < at + 5) return NEEDS;
        ids = argv[at + 1]; quality = argv[at + 2]; out_ids = argv[at + 3]; out_quality = argv[at + 4]; at += 5;
    }
    if (at < argc && !strcmp(argv[at], "pair")) {
        if (argc != at + 3 || !ids || !number(argv[at + 1], &records) || records < 1 || (rule = harc_amd_idmate_rule_parse(argv[at + 2])) < 0) return NEEDS;
        at += 3;
    }
    if (at != argc) return NEEDS;
    const int rc = harc_amd_match_files(P, argv[2], (uint32_t)K, argv[5], ids, quality, argv[6], out_ids, out_quality, records, rule, st, missing, sizeof missing);
    if (rc != 0) return rc;
    printf("[match] %llu motifs, %llu found, %llu of %llu records\n", (ull)st[0], (ull)st[1], (ull)st[2], (ull)st[3]);
    for (const char *p = missing; *p;) { const char *e = strchr(p, '\n'); if (!e) break; printf("[match] not found: %.*s\n", (int)(e - p), p); p = e + 1; }
    return 0;
}

static int do_unpack_range(int, char **argv, harc_amd_params *P)                    // quality_unpack_range, id_unpack_range
{
    uint64_t first = 0, count = 0;
    if (!number(argv[5], &first) || !number(argv[6], &count)) return NEEDS;
    return !strcmp(argv[1], "quality_unpack_range") ? harc_amd_qunpack_range_files(P, argv[2], argv[4], first, count) : harc_amd_idunpack_range_files(P, argv[2], argv[4], first, count);
}

static int do_decoder_range(int argc, char **argv, harc_amd_params *P)              // decoder_range, and decoder_preserve_range with <memory_gb> in front of the first <first>
{
    const bool keep = !strcmp(argv[1], "decoder_preserve_range");
    const int at = keep ? 6 : 5, left = argc - at;
    uint64_t first[2] = { 0, 0 }, count[2] = { 0, 0 };
    if (left != 2 && left != 4) return NEEDS;
    for (int k = 0; k < left / 2; k++) if (!number(argv[at + 2 * k], &first[k]) || !number(argv[at + 2 * k + 1], &count[k])) return NEEDS;
    if (keep) P->decode_memory_gb = atoi(argv[5]);
    return keep ? harc_amd_decoder_preserve_range_files(P, argv[2], atoi(argv[4]), left / 2, first, count) : harc_amd_decoder_range_files(P, argv[2], atoi(argv[4]), left / 2, first, count);
}

static int do_preprocess(int, char **argv, harc_amd_params *) { return harc_amd_preprocess_files(argv[4], argv[2], atoi(argv[3])); }

static int do_compressfq(int argc, char **argv, harc_amd_params *P)
{
    schedule_words(P, argc, argv, 5);
    const int po = argc > 8 && !strcmp(argv[8], "True"), pq = argc > 9 && !strcmp(argv[9], "True");     // preprocess.out's argv[3], argv[4] (harc:50)
    if (!check_word(argc, argv)) return REFUSED;
    return harc_amd_compress_fastq_files_checked(P, argv[4], argv[2], po, pq, argc > 10);
}

static int do_compressfq_pair(int argc, char **argv, harc_amd_params *P)
{
    schedule_words(P, argc, argv, 6);
    if (!check_word(argc, argv)) return REFUSED;
    return harc_amd_compress_fastq_pair_files(P, argv[4], argv[5], argv[2], !strcmp(argv[9], "True"), argc > 10, nullptr);
}

static int do_compressfq_shard(int argc, char **argv, harc_amd_params *P)
{
    schedule_words(P, argc, argv, 5);
    const int po = !strcmp(argv[8], "True"), pq = !strcmp(argv[9], "True"), world = atoi(argv[10]), rank = atoi(argv[11]);
    P->device = argc > 13 ? atoi(argv[13]) : rank;                // one process per GPU: rank r drives device r unless told otherwise
    // [mode] after [device]: "replicate" = design (R) (reads all-gathered, chains partitioned, single-GPU bytes); default: minimizer-bucket shards
    // anything else is refused: a typo must not silently give the archive with the larger consensus
    if (argc > 14 && strcmp(argv[14], "replicate") && strcmp(argv[14], "bucket")) { fprintf(stderr, "compressfq_shard: mode '%s' is neither 'bucket' nor 'replicate'\n", argv[14]); return REFUSED; }
    if (argc > 14 && !strcmp(argv[14], "replicate")) return harc_amd_compress_fastq_replicated_files(P, argv[4], argv[2], po, pq, world, rank, argv[12]);   // reads_per_chain 0
    P->reads_per_chain = 1024;                                    // a bucket shard is fragmented already (multi-GPU)
    return harc_amd_compress_fastq_shard_files(P, argv[4], argv[2], po, pq, world, rank, argv[12]);
}

static int do_decoder(int argc, char **argv, harc_amd_params *P) { return harc_amd_decoder_files(P, argv[2], argc > 4 ? atoi(argv[4]) : 1); }
static int do_decoder_preserve(int argc, char **argv, harc_amd_params *P)
{
    if (argc > 5) P->decode_memory_gb = atoi(argv[5]);            // [memory]: -m of harc:174
    return harc_amd_decoder_preserve_files(P, argv[2], argc > 4 ? atoi(argv[4]) : 1);
}
static int do_stage(int argc, char **argv, harc_amd_params *P)                      // reorder, encoder, compress, pack_order
{
    schedule_words(P, argc, argv, 4);
    return !strcmp(argv[1], "reorder") ? harc_amd_reorder_files(P, argv[2]) : !strcmp(argv[1], "encoder") ? harc_amd_encoder_files(P, argv[2])
           : !strcmp(argv[1], "compress") ? harc_amd_compress_files(P, argv[2]) : harc_amd_pack_order_files(P, argv[2]);
}

// where the read length of the prepared params comes from
enum { RL_100,          // the command reads it from its files, or has no use for it
       RL_WORD,         // argv[3]
       RL_DECODER };    // argv[3] when it is one, else 100: the decoder takes readlen from read_meta.txt (decoder.cpp:324-333)

struct command {
    const char *name;
    int min_argc;       // fewer words: the "needs" line, status 2
    int readlen;        // RL_*
    int device;         // 0: the handler's business; k: argv[k]; -k: argv[k] when it is there
    const char *needs;  // "<name> needs <this>"; none: the commands of the reference's driver, which share main's usage line
    int (*run)(int argc, char **argv, harc_amd_params *P);      // the library's code, or NEEDS / REFUSED / DAMAGED
};

static const command commands[] = {
    // ---- the stages of the reference's driver (the words: top of this file)
    { "reorder", 4, RL_WORD, 0, nullptr, do_stage },
    { "encoder", 4, RL_WORD, 0, nullptr, do_stage },
    { "compress", 4, RL_WORD, 0, nullptr, do_stage },
    { "pack_order", 4, RL_WORD, 0, nullptr, do_stage },
    { "decoder", 4, RL_DECODER, 0, nullptr, do_decoder },
    { "decoder_preserve", 4, RL_DECODER, 0, nullptr, do_decoder_preserve },
    { "preprocess", 5, RL_WORD, 0, "<fastq>", do_preprocess },
    // compressfq: "check" (./harc -c -V): the streams are decoded once before they are written, and output/read.check is written
    { "compressfq", 5, RL_WORD, 0, "<fastq>", do_compressfq },
    // compressfq over two files as one job, the order kept (./harc -c R1 -2 R2 -p): the records of <fastq1>, then those of <fastq2>; output/read.pair records their number
    { "compressfq_pair", 10, RL_WORD, 0, "<fastq1> <fastq2> <num_thr> <num_chains> <num_steps> <preserve_quality> [check]", do_compressfq_pair },
    // one rank of `./harc -c -g <world>` (one process per GPU); behind [device]: [bucket|replicate]
    { "compressfq_shard", 13, RL_WORD, 0, "<fastq> <num_thr> <num_chains> <num_steps> <p> <q> <world> <rank> <comm_spec> [device]", do_compressfq_shard },
    // merge_shards <basedir> <world>: the whole-job files of the archive from the rank parts
    { "merge_shards", 4, RL_100, 0, nullptr, do_merge_shards },
    // ---- ./harc -d -r: decoder and decoder_preserve that write only those lines of their output, one range after the other
    { "decoder_range", 7, RL_100, 0, "<basedir> <ignored> <num_thr_e> <first> <count> [<first> <count>], lines counted from 0", do_decoder_range },
    { "decoder_preserve_range", 8, RL_100, 0, "<basedir> <ignored> <num_thr_e> <memory_gb> <first> <count> [<first> <count>], lines counted from 0", do_decoder_range },
    // ---- ./harc -d -q: lines i of the three files -> record i of the FASTQ file <out>.  bgzf: <out> is that text as BGZF, deflated on the GPU (-z); third: the third
    // line of every record is '+' and its id without the first byte (the archive's read.third names the rule same)
    { "fastq_out", 7, RL_100, 0, "<dna> <ignored> <id> <quality> <out> [bgzf] [third]", do_fastq_out },
    // ... for a paired archive: records [0, n) -> <out1>, [n, 2 n) -> <out2>, the second file's ids made from the first's by <rule> on the GPU (-d -p -q)
    { "fastq_out_pair", 10, RL_100, 0, "<dna> <ignored> <id> <quality> <out1> <out2> <records> <rule> [bgzf] [third]", do_fastq_out_pair },
    // ---- the side files.  quality_pack: the fixed-length lines of <in> -> the packed quality file <out> (./harc -c -q -Q); a fourth word <spec>: their values are
    // mapped first, in device memory (-b <spec>).  quality_unpack: ... and back (./harc -d -q when only X.quality.hq is there)
    { "quality_pack", 5, RL_100, 3, "<in> <device> <out>", do_quality_map },
    { "quality_unpack", 5, RL_100, 3, "<in> <device> <out>", do_quality_unpack },
    // 0 when <spec> names a mapping of quality values (ill8, bin:T:H:L, cap:M, pblock:R), else 2 and the reason
    { "quality_spec", 3, RL_100, 0, "<spec>", do_quality_spec },
    // <quality> with its values mapped -> <out> (./harc -c -q -b <spec>)
    { "quality_map", 6, RL_100, 3, "<quality> <device> <out> <spec>", do_quality_map },
    // the lines of <in> -> the packed id file <out> (./harc -c -q -I), and back (./harc -d -q when only X.id.hi is there)
    { "id_pack", 5, RL_100, 3, "<in> <device> <out>", do_id_pack },
    { "id_unpack", 5, RL_100, 3, "<in> <device> <out>", do_id_unpack },
    // quality_unpack and id_unpack for those lines alone: only the blocks that hold them are read (./harc -d -q -r)
    { "quality_unpack_range", 7, RL_100, 3, "<packed> <device> <out> <first> <count>, lines counted from 0", do_unpack_range },
    { "id_unpack_range", 7, RL_100, 3, "<packed> <device> <out> <first> <count>, lines counted from 0", do_unpack_range },
    // "begin end" on stdout and nothing else: the byte range of lines <first> .. <first> + <count> - 1 of the text file, the newlines counted on the GPU (-d -q -r on a plain X.id)
    { "line_range", 5, RL_100, -5, "<file> <first> <count> [<device>], lines counted from 0", do_line_range },
    // "<rule> <pairs>" on stdout and nothing else: the mate rule (none, same, slash, space) that every pair of lines of the two id files follows
    { "id_mates", 4, RL_100, -4, "<a> <b> [<device>]", do_id_mates },
    // the records whose id line carries a name of the list <names> -> the three <out_*> texts, selected and gathered on the GPU in one process (./harc -d -q -L); "[select] <names>
    // names, <found> found, <selected> of <records> records" on stdout, then up to ten "[select] not found: <name>" lines; 0 also when nothing was selected
    { "records_select", 10, RL_100, 3, "<names> <device> <ids> <dna> <quality> <out_ids> <out_dna> <out_quality> [pair <records> <none|same|slash|space>]", do_records_select },
    // 0 and "<n> motifs" when the rule of harc_amd/csrc/motif.h takes the list <file> with <K> mismatches (0 .. 8), else 2 and the reason, which names the line; no device
    { "motifs_check", 4, RL_100, 0, "<file> <K 0..8>", do_motifs_check },
    // the lines of <dna> whose read matches a motif of the list <motifs>, on either strand, with up to <K> mismatches -> <out_dna>, matched and gathered on the GPU in one
    // process (./harc -d -M); behind q the same records of the two side texts; "[match] <motifs> motifs, <found> found, <selected> of <records> records" on stdout, then up
    // to ten "[match] not found: <motif>" lines; 0 also when nothing was selected
    { "records_match", 7, RL_100, 3, "<motifs> <device> <K 0..8> <dna> <out_dna> [q <ids> <quality> <out_ids> <out_quality>] [pair <records> <none|same|slash|space>]", do_records_match },
    // ---- the streams of the archive: every <in> -> the packed stream file <out>, one after the other on one context (./harc -c -S), and back (./harc -d on .hs members)
    { "streams_pack", 5, RL_100, 2, "<device> <in> <out> [<in> <out> ...]", do_streams },
    { "streams_unpack", 5, RL_100, 2, "<device> <in> <out> [<in> <out> ...]", do_streams },
    // any gzip file -> its text, inflated on the GPU (HARC_AMD_GUNZIP=1 ./harc -c on a .fastq.gz that is not BGZF); one line on stdout: members, chunks, starts found / dropped /
    // repaired, bytes of text
    { "gunzip", 5, RL_100, 3, "<gz> <device> <out>", do_gunzip },
    // ---- ./harc -c -V, -d, -v.  text_digest: "bytes lines D" of the file's text on stdout, 16 hex digits each.  reads_check: "count sum xor bytes lines D" of the decoders'
    // output, read once: the multiset signature of its reads and the digest of its text
    { "text_digest", 3, RL_100, -3, "<file> [<device>]", do_digest },
    { "reads_check", 3, RL_100, -3, "<file> [<device>]", do_digest },
    // ---- the recovery record <out> over the files, erasure-coded on the GPU (./harc -c -P <pct>); one "[recovery]" line on stdout: files, bytes protected, bytes of <out>, blocks, groups
    { "recovery_make", 6, RL_100, 3, "<pct 1..100> <device> <out> <file> [<file> ...]", do_recovery_make },
    // the files the record names, next to it, held against it; one "[recovery]" line per file; 0 when nothing is damaged (./harc -R -n)
    { "recovery_check", 3, RL_100, -3, "<record> [<device>]", do_recovery },
    // ... and the damaged blocks rebuilt in place; 0 when every file verifies in the end (./harc -R)
    { "recovery_repair", 3, RL_100, -3, "<record> [<device>]", do_recovery },
};

int main(int argc, char **argv)
{
    const command *c = nullptr;
    for (const command &k : commands) if (argc >= 2 && !strcmp(argv[1], k.name)) c = &k;
    if (argc < 4 && !(c && c->needs)) { fprintf(stderr, "usage: %s reorder|encoder|compress|pack_order <basedir> <readlen> [num_thr] [num_chains]\n", argv[0]); return 2; }
    if (!c) { fprintf(stderr, "unknown stage %s\n", argv[1]); return 2; }
    if (argc < c->min_argc) { fprintf(stderr, "%s needs %s\n", c->name, c->needs); return 2; }
    // RCCL between processes needs dmabuf IPC on this driver stack (hipIpcGetMemHandle fails otherwise): set before the first HIP call
    // of the process, which is inside the library.  An explicit setting of the caller wins.
    if (!strcmp(c->name, "compressfq_shard")) setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0);
    harc_amd_params P;
    int rl = c->readlen == RL_100 ? 100 : atoi(argv[3]);
    if (c->readlen == RL_DECODER && (rl < 1 || rl > 255)) rl = 100;
    if (harc_amd_default_params(rl, &P) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 1; }
    if (c->device > 0) P.device = atoi(argv[c->device]);
    if (c->device < 0 && argc > -c->device) P.device = atoi(argv[-c->device]);
    const int rc = c->run(argc, argv, &P);
    if (rc == NEEDS) { fprintf(stderr, "%s needs %s\n", c->name, c->needs); return 2; }
    if (rc == REFUSED) return 2;
    if (rc == DAMAGED) return 1;
    if (rc != 0) { fprintf(stderr, "harc_amd_stage %s failed (%d): %s\n", c->name, rc, harc_amd_last_error()); return 1; }   // non-zero aborts `set -e` (harc:2)
    return 0;
}
