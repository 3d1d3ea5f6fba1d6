// main.cpp -- harc_amd_stage: command-line twin of the reference's stage executables.
//   harc_amd_stage reorder  <basedir> <readlen> [num_thr] [num_chains]     == src/reorder.out  <basedir>   (harc:67)
//   harc_amd_stage encoder  <basedir> <readlen> [num_thr] [num_chains]     == src/encoder.out  <basedir>   (harc:69)
//   harc_amd_stage compress <basedir> <readlen> [num_thr] [num_chains]     == both, stage I -> II handed over in HBM
//   harc_amd_stage pack_order <basedir> <readlen>                          == src/pack_order.out <basedir> (harc:112)
//   harc_amd_stage decoder <basedir> <readlen ignored> <num_thr_e>         == src/decoder.out <basedir> <num_thr> <num_thr_e> (harc:188)
//   harc_amd_stage decoder_preserve <basedir> <ignored> <num_thr_e> [memory_gb]   == unpack_order + decoder_preserve + merge_N (harc:174-185, -m = MAX_BIN_SIZE)
//   harc_amd_stage compressfq <basedir> <readlen> <fastq> [num_thr] [num_chains] [num_steps] [preserve_order] [preserve_quality]
//                                                                          == preprocess + reorder + encoder (+ reorder_quality), FASTQ parsed on the GPU
//   harc_amd_stage preprocess <basedir> <readlen> <fastq>                  == src/preprocess.out <fastq> <basedir> .. <readlen> (harc:50)
//   harc_amd_stage compressfq_shard <basedir> <readlen> <fastq> <num_thr> <num_chains> <num_steps> <preserve_order> <preserve_quality>
//                                   <world> <rank> <comm_spec> [device] [replicate]    one rank of `./harc -c -g <world>` (one process per GPU)
//   harc_amd_stage merge_shards <basedir> <world>                          the whole-job files of the archive from the rank parts
//   harc_amd_stage fastq_out <dna> <ignored> <id> <quality> <out> [bgzf]     lines i of the three files -> record i of the FASTQ file <out> (./harc -d -q);
//                                                                          bgzf: <out> is that text as BGZF, deflated on the GPU (./harc -d -q -z)
//                                                                          fastq_out and fastq_out_pair take one more trailing word, third (behind bgzf where both are given): the third
//                                                                          line of every record is '+' and its id without the first byte (the archive's read.third names the rule same)
//   harc_amd_stage quality_pack <quality> <device> <out> [<spec>]          the fixed-length lines of <quality> -> the packed quality file <out> (./harc -c -q -Q);
//                                                                          <spec>: their values are mapped first, in device memory (./harc -c -q -Q -b <spec>)
//   harc_amd_stage quality_spec <spec>                                     0 when <spec> names a mapping of quality values (ill8, bin:T:H:L, cap:M, pblock:R), else 2
//                                                                          and the reason; no device is touched
//   harc_amd_stage quality_map <quality> <device> <out> <spec>             <quality> with its values mapped -> <out> (./harc -c -q -b <spec>)
//   harc_amd_stage quality_unpack <packed> <device> <out>                  ... and back (./harc -d -q when only X.quality.hq is there)
//   harc_amd_stage id_pack <id> <device> <out>                             the lines of <id> -> the packed id file <out> (./harc -c -q -I)
//   harc_amd_stage id_unpack <packed> <device> <out>                       ... and back (./harc -d -q when only X.id.hi is there)
//   harc_amd_stage streams_pack <device> <in> <out> [<in> <out> ...]       every <in> -> the packed stream file <out>, one after the other on one context (./harc -c -S)
//   harc_amd_stage streams_unpack <device> <in> <out> [<in> <out> ...]     ... and back (./harc -d when the archive holds .hs files)
//   harc_amd_stage gunzip <gz> <device> <out>                              any gzip file -> its text, inflated on the GPU (HARC_AMD_GUNZIP=1 ./harc -c on a .fastq.gz that is not BGZF);
//                                                                          one line on stdout: members, chunks, starts found / dropped / repaired, bytes of text
//   harc_amd_stage text_digest <file> [<device>]                          "bytes lines D" of the file's text on stdout, 16 hex digits each (./harc -c -V, -d, -v)
//   harc_amd_stage reads_check <dna> [<device>]                            "count sum xor bytes lines D" of the decoders' output, read once: the multiset signature
//                                                                          of its reads and the digest of its text (./harc -d, -v on an archive made with -V)
//   harc_amd_stage compressfq_pair <basedir> <readlen> <fastq1> <fastq2> <num_thr> <num_chains> <num_steps> <preserve_quality> [check]
//                                                                          compressfq over two files as one job, the order kept (./harc -c R1 -2 R2 -p): the records of
//                                                                          <fastq1>, then those of <fastq2>; output/read.pair records their number
//   harc_amd_stage id_mates <a> <b> [<device>]                             "<rule> <pairs>" on stdout and nothing else: the mate rule (none, same, slash, space) that every
//                                                                          pair of lines of the two id files follows
//   harc_amd_stage fastq_out_pair <dna> <ignored> <id> <quality> <out1> <out2> <records> <rule> [bgzf]
//                                                                          fastq_out for a paired archive: records [0, n) -> <out1>, [n, 2 n) -> <out2>, the second file's ids
//                                                                          made from the first's by <rule> on the GPU (./harc -d -p -q)
//   harc_amd_stage line_range <file> <first> <count> [<device>]            "begin end" on stdout and nothing else: the byte range of lines <first> .. <first> + <count> - 1 of the
//                                                                          text file, the newlines counted on the GPU (./harc -d -q -r on a plain X.id)
//   harc_amd_stage quality_unpack_range <packed> <device> <out> <first> <count>   quality_unpack for those lines alone: only the blocks that hold them are read (./harc -d -q -r)
//   harc_amd_stage id_unpack_range <packed> <device> <out> <first> <count>        ... and id_unpack
//   harc_amd_stage decoder_range <basedir> <ignored> <num_thr_e> <first> <count> [<first> <count>]
//                                                                          decoder that writes only those lines of its output, one range after the other (./harc -d -r)
//   harc_amd_stage decoder_preserve_range <basedir> <ignored> <num_thr_e> <memory_gb> <first> <count> [<first> <count>]     ... and decoder_preserve (./harc -d -p -r)
//   harc_amd_stage recovery_make <pct> <device> <out> <file> [<file> ...]  the recovery record <out> over the files, erasure-coded on the GPU (./harc -c -P <pct>); one "[recovery]" line
//                                                                          on stdout: files, bytes protected, bytes of <out>, blocks, groups
//   harc_amd_stage recovery_check <record> [<device>]                      the files the record names, next to it, held against it; one "[recovery]" line per file; 0 when nothing
//                                                                          is damaged (./harc -R -n)
//   harc_amd_stage recovery_repair <record> [<device>]                     ... and the damaged blocks rebuilt in place; 0 when every file verifies in the end (./harc -R)
//   harc_amd_stage records_select <names> <device> <ids> <dna> <quality> <out_ids> <out_dna> <out_quality> [pair <records> <rule>]
//                                                                          the records whose id line carries a name of the list <names> -> the three <out_*> texts, selected and
//                                                                          gathered on the GPU in one process (./harc -d -q -L); "[select] <names> names, <found> found, <selected>
//                                                                          of <records> records" on stdout, then up to ten "[select] not found: <name>" lines; 0 also when nothing
//                                                                          was selected
// (every <first> above counts lines from 0; ./harc -r counts from 1)
// compressfq takes one more trailing argument, "check" (./harc -c -V): the streams are decoded once before they are written, and output/read.check is written.
// readlen / num_thr arrive as arguments instead of the compile-time macros of src/config.h (harc:52-63).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/harc_amd.h"

// what a mapping of quality values did, one line on stdout
static void print_qmap(const char *spec, const harc_amd_qmap_stats *st)
{
    printf("[qmap] %s: %llu values, %llu changed, mean absolute change %.3f, max change %u, distinct values %u -> %u\n", spec, (unsigned long long)st->values,
           (unsigned long long)st->changed, st->values ? (double)st->sum_abs / (double)st->values : 0.0, st->max_abs, st->distinct_in, st->distinct_out);
}

// the optional words behind the fixed arguments of fastq_out and fastq_out_pair: [bgzf] [third], in that order and nothing else
static bool trailing_words(int argc, char **argv, int at, int *bgzf, int *third)
{
    *bgzf = *third = 0;
    if (at < argc && !strcmp(argv[at], "bgzf")) { *bgzf = 1; at++; }
    if (at < argc && !strcmp(argv[at], "third")) { *third = 1; at++; }
    return at == argc;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "quality_spec")) {
        harc_amd_qmap M;
        if (argc != 3) { fprintf(stderr, "quality_spec needs <spec>\n"); return 2; }
        if (harc_amd_qmap_parse(argv[2], &M) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 2; }
        return 0;
    }
    if (argc >= 2 && (!strcmp(argv[1], "text_digest") || !strcmp(argv[1], "reads_check"))) {
        if (argc < 3) { fprintf(stderr, "%s needs <file> [<device>]\n", argv[1]); return 2; }
        harc_amd_params PC;
        if (harc_amd_default_params(100, &PC) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 1; }
        if (argc > 3) PC.device = atoi(argv[3]);
        uint64_t sig[3] = { 0, 0, 0 }, t[3] = { 0, 0, 0 };
        const bool reads = !strcmp(argv[1], "reads_check");
        const int rcc = reads ? harc_amd_reads_check_files(&PC, argv[2], sig, t) : harc_amd_text_digest_files(&PC, argv[2], t);
        if (rcc != 0) { fprintf(stderr, "harc_amd_stage %s failed (%d): %s\n", argv[1], rcc, harc_amd_last_error()); return 1; }
        if (reads) printf("%016llx %016llx %016llx ", (unsigned long long)sig[0], (unsigned long long)sig[1], (unsigned long long)sig[2]);
        printf("%016llx %016llx %016llx\n", (unsigned long long)t[0], (unsigned long long)t[1], (unsigned long long)t[2]);
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "id_mates")) {
        if (argc < 4) { fprintf(stderr, "id_mates needs <a> <b> [<device>]\n"); return 2; }
        harc_amd_params PM;
        if (harc_amd_default_params(100, &PM) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 1; }
        if (argc > 4) PM.device = atoi(argv[4]);
        int32_t rule = 0; uint64_t pairs = 0;
        const int rcm = harc_amd_idmate_rule_files(&PM, argv[2], argv[3], &rule, &pairs);
        if (rcm != 0) { fprintf(stderr, "harc_amd_stage id_mates failed (%d): %s\n", rcm, harc_amd_last_error()); return 1; }
        printf("%s %llu\n", harc_amd_idmate_rule_name(rule), (unsigned long long)pairs);
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "recovery_make")) {
        char *end = nullptr;
        const long pct = argc > 2 ? strtol(argv[2], &end, 10) : 0;
        if (argc < 6 || !*argv[2] || *end || pct < 1 || pct > 100) { fprintf(stderr, "recovery_make needs <pct 1..100> <device> <out> <file> [<file> ...]\n"); return 2; }
        harc_amd_params PR;
        if (harc_amd_default_params(100, &PR) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 1; }
        PR.device = atoi(argv[3]);
        uint64_t st[5] = { 0, 0, 0, 0, 0 };
        const int rcr = harc_amd_recovery_make_files(&PR, argc - 5, (const char *const *)(argv + 5), (uint32_t)pct, argv[4], st);
        if (rcr != 0) { fprintf(stderr, "harc_amd_stage recovery_make failed (%d): %s\n", rcr, harc_amd_last_error()); return 1; }
        printf("[recovery] %llu files, %llu bytes protected, %llu bytes of %s, %llu blocks, %llu groups\n", (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2],
               argv[4], (unsigned long long)st[3], (unsigned long long)st[4]);
        return 0;
    }
    if (argc >= 2 && (!strcmp(argv[1], "recovery_check") || !strcmp(argv[1], "recovery_repair"))) {
        if (argc < 3) { fprintf(stderr, "%s needs <record> [<device>]\n", argv[1]); return 2; }
        harc_amd_params PR;
        if (harc_amd_default_params(100, &PR) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 1; }
        if (argc > 3) PR.device = atoi(argv[3]);
        static char report[1 << 16];
        int32_t status = 1;
        report[0] = 0;
        const int rcr = !strcmp(argv[1], "recovery_check") ? harc_amd_recovery_check_files(&PR, argv[2], report, sizeof report, &status)
                                                           : harc_amd_recovery_repair_files(&PR, argv[2], report, sizeof report, &status);
        fputs(report, stdout);
        if (rcr != 0) { fprintf(stderr, "harc_amd_stage %s failed (%d): %s\n", argv[1], rcr, harc_amd_last_error()); return 1; }
        return status ? 1 : 0;
    }
    if (argc < 4) { fprintf(stderr, "usage: %s reorder|encoder|compress|pack_order <basedir> <readlen> [num_thr] [num_chains]\n", argv[0]); return 2; }
    // RCCL between processes needs dmabuf IPC on this driver stack (hipIpcGetMemHandle fails otherwise): set before the first HIP call
    // of the process, which is inside the library.  An explicit setting of the caller wins.
    if (!strcmp(argv[1], "compressfq_shard")) setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0);
    if (!strcmp(argv[1], "merge_shards")) {
        const int rcm = harc_amd_merge_shard_files(argv[2], atoi(argv[3]));
        if (rcm != 0) { fprintf(stderr, "harc_amd_stage merge_shards failed (%d): %s\n", rcm, harc_amd_last_error()); return 1; }
        return 0;
    }
    if (!strcmp(argv[1], "fastq_out")) {                          // the read length is the first line's of <dna>
        if (argc < 7) { fprintf(stderr, "fastq_out needs <dna> <ignored> <id> <quality> <out> [bgzf] [third]\n"); return 2; }
        int bgzf = 0, third = 0;
        if (!trailing_words(argc, argv, 7, &bgzf, &third)) { fprintf(stderr, "fastq_out: behind <out> only 'bgzf', 'third' or 'bgzf third' can follow (got '%s')\n", argv[argc - 1]); return 2; }
        harc_amd_params PF;
        if (harc_amd_default_params(100, &PF) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 1; }
        const int rcf = third ? harc_amd_fastq_assemble_third_files(&PF, argv[2], argv[4], argv[5], argv[6], bgzf, HARC_AMD_THIRD_SAME)
                        : bgzf ? harc_amd_fastq_assemble_files_ex(&PF, argv[2], argv[4], argv[5], argv[6], 1) : harc_amd_fastq_assemble_files(&PF, argv[2], argv[4], argv[5], argv[6]);
        if (rcf != 0) { fprintf(stderr, "harc_amd_stage fastq_out failed (%d): %s\n", rcf, harc_amd_last_error()); return 1; }
        return 0;
    }
    if (!strcmp(argv[1], "fastq_out_pair")) {
        if (argc < 10) { fprintf(stderr, "fastq_out_pair needs <dna> <ignored> <id> <quality> <out1> <out2> <records> <rule> [bgzf] [third]\n"); return 2; }
        int bgzf = 0, third = 0;
        if (!trailing_words(argc, argv, 10, &bgzf, &third)) { fprintf(stderr, "fastq_out_pair: behind <rule> only 'bgzf', 'third' or 'bgzf third' can follow (got '%s')\n", argv[argc - 1]); return 2; }
        char *end = nullptr;
        const unsigned long long records = strtoull(argv[8], &end, 10);
        if (!*argv[8] || *end) { fprintf(stderr, "fastq_out_pair: <records> must be a decimal number (got '%s')\n", argv[8]); return 2; }
        const int32_t rule = harc_amd_idmate_rule_parse(argv[9]);
        if (rule < 0) { fprintf(stderr, "fastq_out_pair: <rule> must be none, same, slash or space (got '%s')\n", argv[9]); return 2; }
        harc_amd_params PF;
        if (harc_amd_default_params(100, &PF) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 1; }
        const int rcf = third ? harc_amd_fastq_assemble_third_pair_files(&PF, argv[2], argv[4], argv[5], argv[6], argv[7], records, rule, bgzf, HARC_AMD_THIRD_SAME)
                              : harc_amd_fastq_assemble_pair_files(&PF, argv[2], argv[4], argv[5], argv[6], argv[7], records, rule, bgzf);
        if (rcf != 0) { fprintf(stderr, "harc_amd_stage fastq_out_pair failed (%d): %s\n", rcf, harc_amd_last_error()); return 1; }
        return 0;
    }
    if (!strcmp(argv[1], "quality_pack") || !strcmp(argv[1], "quality_unpack")) {     // the read length is in the file
        if (argc < 5) { fprintf(stderr, "%s needs <in> <device> <out>\n", argv[1]); return 2; }
        harc_amd_params PQ;
        if (harc_amd_default_params(100, &PQ) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 1; }
        PQ.device = atoi(argv[3]);
        if (!strcmp(argv[1], "quality_pack") && argc > 5) {         // the values mapped in front of the coder
            harc_amd_qmap M; harc_amd_qmap_stats ST;
            if (harc_amd_qmap_parse(argv[5], &M) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 2; }
            const int rcm = harc_amd_qpack_files_ex(&PQ, argv[2], argv[4], &M, &ST);
            if (rcm != 0) { fprintf(stderr, "harc_amd_stage %s failed (%d): %s\n", argv[1], rcm, harc_amd_last_error()); return 1; }
            print_qmap(argv[5], &ST);
            return 0;
        }
        const int rcq = !strcmp(argv[1], "quality_pack") ? harc_amd_qpack_files(&PQ, argv[2], argv[4]) : harc_amd_qunpack_files(&PQ, argv[2], argv[4]);
        if (rcq != 0) { fprintf(stderr, "harc_amd_stage %s failed (%d): %s\n", argv[1], rcq, harc_amd_last_error()); return 1; }
        return 0;
    }
    if (!strcmp(argv[1], "quality_map")) {
        if (argc < 6) { fprintf(stderr, "quality_map needs <quality> <device> <out> <spec>\n"); return 2; }
        harc_amd_qmap M; harc_amd_qmap_stats ST;
        if (harc_amd_qmap_parse(argv[5], &M) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 2; }
        harc_amd_params PM;
        if (harc_amd_default_params(100, &PM) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 1; }
        PM.device = atoi(argv[3]);
        const int rcm = harc_amd_qmap_files(&PM, argv[2], argv[4], &M, &ST);
        if (rcm != 0) { fprintf(stderr, "harc_amd_stage quality_map failed (%d): %s\n", rcm, harc_amd_last_error()); return 1; }
        print_qmap(argv[5], &ST);
        return 0;
    }
    if (!strcmp(argv[1], "gunzip")) {
        if (argc < 5) { fprintf(stderr, "gunzip needs <gz> <device> <out>\n"); return 2; }
        harc_amd_params PG; harc_amd_gunzip_stats GS;
        if (harc_amd_default_params(100, &PG) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 1; }
        PG.device = atoi(argv[3]);
        const int rcg = harc_amd_gunzip_files(&PG, argv[2], argv[4], &GS);
        if (rcg != 0) { fprintf(stderr, "harc_amd_stage gunzip failed (%d): %s\n", rcg, harc_amd_last_error()); return 1; }
        printf("[gunzip] %llu members, %llu chunks, %llu starts found, %llu dropped, %llu repaired, %llu bytes of text\n", (unsigned long long)GS.members, (unsigned long long)GS.chunks,
               (unsigned long long)GS.starts_found, (unsigned long long)GS.starts_dropped, (unsigned long long)GS.repair_walks, (unsigned long long)GS.text_bytes);
        return 0;
    }
    if (!strcmp(argv[1], "streams_pack") ||!strcmp(argv[1], "streams_unpack")) {
        if (argc < 5 || (argc - 3) % 2) { fprintf(stderr, "%s needs <device> <in> <out> [<in> <out> ...]\n", argv[1]); return 2; }
        harc_amd_params PS;
        if (harc_amd_default_params(100, &PS) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 1; }
        PS.device = atoi(argv[2]);
        const int np = (argc - 3) / 2;
        const char **in = (const char **)malloc(sizeof(char *) * 2 * (size_t)np), **out = in + np;
        if (!in) return 1;
        for (int k = 0; k < np; k++) { in[k] = argv[3 + 2 * k]; out[k] = argv[4 + 2 * k]; }
        const int rcs = !strcmp(argv[1], "streams_pack") ? harc_amd_spack_file_list(&PS, np, in, out) : harc_amd_sunpack_file_list(&PS, np, in, out);
        free(in);
        if (rcs != 0) { fprintf(stderr, "harc_amd_stage %s failed (%d): %s\n", argv[1], rcs, harc_amd_last_error()); return 1; }
        return 0;
    }
    if (!strcmp(argv[1], "id_pack") || !strcmp(argv[1], "id_unpack")) {
        if (argc < 5) { fprintf(stderr, "%s needs <in> <device> <out>\n", argv[1]); return 2; }
        harc_amd_params PI;
        if (harc_amd_default_params(100, &PI) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 1; }
        PI.device = atoi(argv[3]);
        const int rci = !strcmp(argv[1], "id_pack") ? harc_amd_idpack_files(&PI, argv[2], argv[4]) : harc_amd_idunpack_files(&PI, argv[2], argv[4]);
        if (rci != 0) { fprintf(stderr, "harc_amd_stage %s failed (%d): %s\n", argv[1], rci, harc_amd_last_error()); return 1; }
        return 0;
    }
    // a decimal number that fits 64 bits and nothing else
    auto number = [](const char *s, uint64_t *v) { char *end = nullptr; if (!*s || *s == '-' || *s == '+') return false; *v = strtoull(s, &end, 10); return *end == 0; };
    if (!strcmp(argv[1], "line_range")) {
        uint64_t first = 0, count = 0, r[2] = { 0, 0 };
        if (argc < 5 || !number(argv[3], &first) || !number(argv[4], &count)) { fprintf(stderr, "line_range needs <file> <first> <count> [<device>], lines counted from 0\n"); return 2; }
        harc_amd_params PL;
        if (harc_amd_default_params(100, &PL) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 1; }
        if (argc > 5) PL.device = atoi(argv[5]);
        const int rcl = harc_amd_line_range_files(&PL, argv[2], first, count, r);
        if (rcl != 0) { fprintf(stderr, "harc_amd_stage line_range failed (%d): %s\n", rcl, harc_amd_last_error()); return 1; }
        printf("%llu %llu\n", (unsigned long long)r[0], (unsigned long long)r[1]);
        return 0;
    }
    if (!strcmp(argv[1], "records_select")) {
        // records_select <names> <device> <ids> <dna> <quality> <out_ids> <out_dna> <out_quality> [pair <records> <rule>]
        uint64_t records = 0; int32_t rule = 0;
        bool ok = argc == 10 || argc == 13;
        if (ok && argc == 13) { ok = !strcmp(argv[10], "pair") && number(argv[11], &records) && records >= 1; rule = ok ? harc_amd_idmate_rule_parse(argv[12]) : -1; ok = ok && rule >= 0; }
        if (!ok) { fprintf(stderr, "records_select needs <names> <device> <ids> <dna> <quality> <out_ids> <out_dna> <out_quality> [pair <records> <none|same|slash|space>]\n"); return 2; }
        harc_amd_params PS;
        if (harc_amd_default_params(100, &PS) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 1; }
        PS.device = atoi(argv[3]);
        uint64_t st[4] = { 0, 0, 0, 0 };
        static char missing[1 << 16];
        const int rcs = harc_amd_select_files(&PS, argv[2], argv[4], argv[5], argv[6], argv[7], argv[8], argv[9], records, rule, st, missing, sizeof missing);
        if (rcs != 0) { fprintf(stderr, "harc_amd_stage records_select failed (%d): %s\n", rcs, harc_amd_last_error()); return 1; }
        printf("[select] %llu names, %llu found, %llu of %llu records\n", (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2], (unsigned long long)st[3]);
        for (const char *p = missing; *p;) { const char *e = strchr(p, '\n'); if (!e) break; printf("[select] not found: %.*s\n", (int)(e - p), p); p = e + 1; }
        return 0;
    }
    if (!strcmp(argv[1], "quality_unpack_range") || !strcmp(argv[1], "id_unpack_range")) {
        uint64_t first = 0, count = 0;
        if (argc < 7 || !number(argv[5], &first) || !number(argv[6], &count)) { fprintf(stderr, "%s needs <packed> <device> <out> <first> <count>, lines counted from 0\n", argv[1]); return 2; }
        harc_amd_params PR;
        if (harc_amd_default_params(100, &PR) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 1; }
        PR.device = atoi(argv[3]);
        const int rcr = !strcmp(argv[1], "quality_unpack_range") ? harc_amd_qunpack_range_files(&PR, argv[2], argv[4], first, count) : harc_amd_idunpack_range_files(&PR, argv[2], argv[4], first, count);
        if (rcr != 0) { fprintf(stderr, "harc_amd_stage %s failed (%d): %s\n", argv[1], rcr, harc_amd_last_error()); return 1; }
        return 0;
    }
    if (!strcmp(argv[1], "decoder_range") || !strcmp(argv[1], "decoder_preserve_range")) {
        // decoder_range <basedir> <ignored> <num_thr_e> <first> <count> [<first> <count>]; decoder_preserve_range has <memory_gb> in front of the first <first>
        const bool keep = !strcmp(argv[1], "decoder_preserve_range");
        const int at = keep ? 6 : 5, left = argc - at;
        uint64_t first[2] = { 0, 0 }, count[2] = { 0, 0 };
        bool ok = left == 2 || left == 4;
        for (int k = 0; ok && k < left / 2; k++) ok = number(argv[at + 2 * k], &first[k]) && number(argv[at + 2 * k + 1], &count[k]);
        if (!ok) { fprintf(stderr, "%s needs <basedir> <ignored> <num_thr_e> %s<first> <count> [<first> <count>], lines counted from 0\n", argv[1], keep ? "<memory_gb> " : ""); return 2; }
        harc_amd_params PD;
        if (harc_amd_default_params(100, &PD) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 1; }
        if (keep) PD.decode_memory_gb = atoi(argv[5]);
        const int rcd = keep ? harc_amd_decoder_preserve_range_files(&PD, argv[2], atoi(argv[4]), left / 2, first, count) : harc_amd_decoder_range_files(&PD, argv[2], atoi(argv[4]), left / 2, first, count);
        if (rcd != 0) { fprintf(stderr, "harc_amd_stage %s failed (%d): %s\n", argv[1], rcd, harc_amd_last_error()); return 1; }
        return 0;
    }
    harc_amd_params P;
    int rl = atoi(argv[3]);
    if (!strncmp(argv[1], "decoder", 7) && (rl < 1 || rl > 255)) rl = 100;     // the decoder takes readlen from read_meta.txt (decoder.cpp:324-333)
    if (harc_amd_default_params(rl, &P) != 0) { fprintf(stderr, "%s\n", harc_amd_last_error()); return 1; }
    if (strcmp(argv[1], "preprocess") && strncmp(argv[1], "decoder", 7) && strncmp(argv[1], "compressfq", 10)) {
        if (argc > 4) P.num_thr = atoi(argv[4]);
        if (argc > 5) P.num_chains = atoi(argv[5]);
        if (argc > 6) P.num_steps = atoi(argv[6]);
    }
    int rc;
    if (!strcmp(argv[1], "preprocess")) { if (argc < 5) { fprintf(stderr, "preprocess needs <fastq>\n"); return 2; } rc = harc_amd_preprocess_files(argv[4], argv[2], atoi(argv[3])); }
    else if (!strcmp(argv[1], "compressfq")) {                    // compressfq <basedir> <readlen> <fastq> [num_thr] [num_chains] [num_steps]
        if (argc < 5) { fprintf(stderr, "compressfq needs <fastq>\n"); return 2; }
        if (argc > 5) P.num_thr = atoi(argv[5]);
        if (argc > 6) P.num_chains = atoi(argv[6]);
        if (argc > 7) P.num_steps = atoi(argv[7]);
        const int po = argc > 8 && !strcmp(argv[8], "True"), pq = argc > 9 && !strcmp(argv[9], "True");     // preprocess.out's argv[3], argv[4] (harc:50)
        if (argc > 10 && strcmp(argv[10], "check")) { fprintf(stderr, "compressfq: the argument behind <preserve_quality> can only be 'check' (got '%s')\n", argv[10]); return 2; }
        rc = harc_amd_compress_fastq_files_checked(&P, argv[4], argv[2], po, pq, argc > 10);
    }
    else if (!strcmp(argv[1], "compressfq_pair")) {
        if (argc < 10) { fprintf(stderr, "compressfq_pair needs <fastq1> <fastq2> <num_thr> <num_chains> <num_steps> <preserve_quality> [check]\n"); return 2; }
        P.num_thr = atoi(argv[6]); P.num_chains = atoi(argv[7]); P.num_steps = atoi(argv[8]);
        if (argc > 10 && strcmp(argv[10], "check")) { fprintf(stderr, "compressfq_pair: the argument behind <preserve_quality> can only be 'check' (got '%s')\n", argv[10]); return 2; }
        rc = harc_amd_compress_fastq_pair_files(&P, argv[4], argv[5], argv[2], !strcmp(argv[9], "True"), argc > 10, nullptr);
    }
    else if (!strcmp(argv[1], "compressfq_shard")) {
        if (argc < 13) { fprintf(stderr, "compressfq_shard needs <fastq> <num_thr> <num_chains> <num_steps> <p> <q> <world> <rank> <comm_spec> [device]\n"); return 2; }
        P.num_thr = atoi(argv[5]); P.num_chains = atoi(argv[6]); P.num_steps = atoi(argv[7]);
        const int po = !strcmp(argv[8], "True"), pq = !strcmp(argv[9], "True"), world = atoi(argv[10]), rank = atoi(argv[11]);
        P.device = argc > 13 ? atoi(argv[13]) : rank;                 // one process per GPU: rank r drives device r unless told otherwise
        P.reads_per_chain = 1024;                                     // a bucket shard is fragmented already (multi-GPU)
        // [mode] after [device]: "replicate" = design (R) (reads all-gathered, chains partitioned, single-GPU bytes); default: minimizer-bucket shards
        // anything else is refused: a typo must not silently give the archive with the larger consensus
        if (argc > 14 && strcmp(argv[14], "replicate") && strcmp(argv[14], "bucket")) { fprintf(stderr, "compressfq_shard: mode '%s' is neither 'bucket' nor 'replicate'\n", argv[14]); return 2; }
        const bool repl = argc > 14 && !strcmp(argv[14], "replicate");
        if (repl) { P.reads_per_chain = 0; rc = harc_amd_compress_fastq_replicated_files(&P, argv[4], argv[2], po, pq, world, rank, argv[12]); }
        else rc = harc_amd_compress_fastq_shard_files(&P, argv[4], argv[2], po, pq, world, rank, argv[12]);
    }
    else if (!strcmp(argv[1], "decoder_preserve")) { if (argc > 5) P.decode_memory_gb = atoi(argv[5]); rc = harc_amd_decoder_preserve_files(&P, argv[2], argc > 4 ? atoi(argv[4]) : 1); }   // [memory]: -m of harc:174
    else if (!strcmp(argv[1], "decoder")) rc = harc_amd_decoder_files(&P, argv[2], argc > 4 ? atoi(argv[4]) : 1);
    else if (!strcmp(argv[1], "reorder")) rc = harc_amd_reorder_files(&P, argv[2]);
    else if (!strcmp(argv[1], "encoder")) rc = harc_amd_encoder_files(&P, argv[2]);
    else if (!strcmp(argv[1], "compress")) rc = harc_amd_compress_files(&P, argv[2]);
    else if (!strcmp(argv[1], "pack_order")) rc = harc_amd_pack_order_files(&P, argv[2]);
    else { fprintf(stderr, "unknown stage %s\n", argv[1]); return 2; }
    if (rc != 0) { fprintf(stderr, "harc_amd_stage %s failed (%d): %s\n", argv[1], rc, harc_amd_last_error()); return 1; }   // non-zero aborts `set -e` (harc:2)
    return 0;
}
