// files.cpp -- the reference's stage programs as library calls with the same file contract:
//   reorder.out <basedir>    src/reorder.cpp:100-131   reads  output/input_clean.dna, output/numreads.bin
//                                                       writes temp.dna, temp.dna.singleton, read_rev.txt, tempflag.txt,
//                                                              temppos.txt, read_order.bin, read_order.bin.singleton
//   encoder.out <basedir>    src/encoder.cpp:108-152   reads  the files above + input_N.dna
//                                                       writes read_{seq,pos,noise,noisepos,rev}.txt.<e>(+.tail), read_singleton.txt(+.tail),
//                                                              read_order.bin, read_order_N_pe.bin, input_N.dna (rewritten), read_meta.txt
//   pack_order.out <basedir> src/pack_order.cpp:11-77  rewrites read_order.bin, writes read_order.bin.tail
#include "fileio.h"

static int load_clean(harc_amd_ctx *c, const std::string &od)
{
    const int L = c->P.readlen;
    std::vector<char> nb, dna;
    if (!slurp_file(od + "numreads.bin", nb, true) || nb.size() < 4) { harc_set_error("numreads.bin missing or short"); return HARC_AMD_EIO; }
    uint32_t N; memcpy(&N, nb.data(), 4);                                          // reorder.cpp:112-113
    if (!slurp_file(od + "input_clean.dna", dna, true)) return HARC_AMD_EIO;
    if (dna.size() < (size_t)N * (L + 1)) { harc_set_error("input_clean.dna holds fewer than %u lines of %d bases", N, L); return HARC_AMD_EIO; }
    return harc_amd_set_reads_ascii(c, dna.data(), N, (uint32_t)L + 1);             // (readlen+1) stride, reorder.cpp:252
}
static int load_N(harc_amd_ctx *c, const std::string &od)
{
    const int L = c->P.readlen;
    std::vector<char> n;
    if (!slurp_file(od + "input_N.dna", n, false)) return HARC_AMD_EIO;
    return harc_amd_set_nreads_ascii(c, n.data(), (uint32_t)(n.size() / (L + 1)), (uint32_t)L + 1);   // encoder.cpp:804-808
}
static int write_stage1(harc_amd_ctx *c, const std::string &od)
{
    RC_TRY(spit_stream(c, HARC_AMD_S1_DNA, 0, od + "temp.dna"));
    RC_TRY(spit_stream(c, HARC_AMD_S1_DNA_SINGLETON, 0, od + "temp.dna.singleton"));
    RC_TRY(spit_stream(c, HARC_AMD_S1_RC, 0, od + "read_rev.txt"));
    RC_TRY(spit_stream(c, HARC_AMD_S1_FLAG, 0, od + "tempflag.txt"));
    RC_TRY(spit_stream(c, HARC_AMD_S1_POS, 0, od + "temppos.txt"));
    RC_TRY(spit_stream(c, HARC_AMD_S1_ORDER, 0, od + "read_order.bin"));
    RC_TRY(spit_stream(c, HARC_AMD_S1_ORDER_SINGLETON, 0, od + "read_order.bin.singleton"));
    return HARC_AMD_OK;
}
// ---- the archive's stage-II files, stated once: the per-shard family read_{seq,pos,noise,noisepos,rev}.txt.<first_shard + e> (+ .tail) of
// encoder.cpp:190-196, then the six files that exist once per job.
// The family goes stream by stream, the largest first: when HARC_AMD_READY_FD names an open descriptor (./harc passes a pipe), the name of every stream is
// written to it as soon as all its shard files are closed, and ./harc starts that stream's stage-III coder (harc:102-109) while the next
// stream is still being written.
static void announce_stream(const char *stem)
{
    const char *e = getenv("HARC_AMD_READY_FD");
    if (!e) return;
    const int fd = atoi(e);
    if (fd < 3) return;
    const std::string line = std::string(stem) + "\n";
    (void)!write(fd, line.data(), line.size());
}
// the stream files of the context's encoder shards [e_lo, e_hi) (e_hi < 0: all) as read_*.txt.<first_shard + e>
int write_shard_family(harc_amd_ctx *c, const std::string &od, int first_shard, int e_lo, int e_hi)
{
    if (e_hi < 0) e_hi = c->P.num_thr;
    static const struct { int id; const char *name; int tail; } files[] = {
        { HARC_AMD_S2_SEQ, "read_seq", HARC_AMD_S2_SEQ_TAIL }, { HARC_AMD_S2_POS, "read_pos", -1 }, { HARC_AMD_S2_NOISE, "read_noise", -1 },
        { HARC_AMD_S2_NOISEPOS, "read_noisepos", -1 }, { HARC_AMD_S2_REV, "read_rev", HARC_AMD_S2_REV_TAIL } };
    for (auto &fd : files) {
        for (int e = e_lo; e < e_hi; e++) {
            const std::string path = od + fd.name + ".txt." + std::to_string(first_shard + e);
            RC_TRY(spit_stream(c, fd.id, e, path));
            if (fd.tail >= 0) RC_TRY(spit_stream(c, fd.tail, e, path + ".tail"));
        }
        if (first_shard == 0) announce_stream(fd.name);
    }
    return HARC_AMD_OK;
}
int write_whole_job_files(harc_amd_ctx *c, const std::string &od)
{
    static const struct { int id; const char *name; } whole[] = {
        { HARC_AMD_S2_ORDER, "read_order.bin" }, { HARC_AMD_S2_ORDER_N_PE, "read_order_N_pe.bin" }, { HARC_AMD_S2_INPUT_N, "input_N.dna" },
        { HARC_AMD_S2_META, "read_meta.txt" }, { HARC_AMD_S2_SINGLETON, "read_singleton.txt" }, { HARC_AMD_S2_SINGLETON_TAIL, "read_singleton.txt.tail" } };
    for (auto &fd : whole) RC_TRY(spit_stream(c, fd.id, 0, od + fd.name));
    return HARC_AMD_OK;
}
static int write_stage2(harc_amd_ctx *c, const std::string &od)
{
    RC_TRY(write_shard_family(c, od, 0, 0, -1));
    return write_whole_job_files(c, od);
}

extern "C" int harc_amd_reorder_files(const harc_amd_params *params, const char *basedir)
{
    if (!params || !basedir) return HARC_AMD_EINVAL;
    CtxGuard g; RC_TRY(harc_amd_create(params, &g.c));
    const std::string od = std::string(basedir) + "/output/";
    RC_TRY(load_clean(g.c, od));
    RC_TRY(harc_amd_reorder(g.c));
    RC_TRY(write_stage1(g.c, od));
    harc_amd_counters C; harc_amd_get_counters(g.c, &C);
    printf("Reordering done, %llu were unmatched\n", (unsigned long long)C.unmatched);                 // reorder.cpp:701
    return HARC_AMD_OK;
}

extern "C" int harc_amd_encoder_files(const harc_amd_params *params, const char *basedir)
{
    if (!params || !basedir) return HARC_AMD_EINVAL;
    CtxGuard g; RC_TRY(harc_amd_create(params, &g.c));
    const int L = params->readlen;
    const std::string od = std::string(basedir) + "/output/";
    std::vector<char> dna, flag, pos, order, rc, dna_s, order_s;
    if (!slurp_file(od + "temp.dna", dna, true) || !slurp_file(od + "tempflag.txt", flag, true) || !slurp_file(od + "temppos.txt", pos, true) ||
        !slurp_file(od + "read_order.bin", order, true) || !slurp_file(od + "read_rev.txt", rc, true) ||
        !slurp_file(od + "temp.dna.singleton", dna_s, true) || !slurp_file(od + "read_order.bin.singleton", order_s, true)) return HARC_AMD_EIO;
    const uint32_t M = (uint32_t)(order.size() / 4), S = (uint32_t)(dna_s.size() / (L + 1));           // encoder.cpp:781-803
    if (dna.size() < (size_t)M * (L + 1) || flag.size() < M || pos.size() < M || rc.size() < M || order_s.size() < (size_t)S * 4) {
        harc_set_error("stage-I files are inconsistent"); return HARC_AMD_EIO;
    }
    RC_TRY(harc_amd_set_stage1_streams(g.c, dna.data(), (const uint8_t *)flag.data(), (const uint8_t *)pos.data(), (const uint32_t *)order.data(),
                                       (const uint8_t *)rc.data(), M, dna_s.data(), (const uint32_t *)order_s.data(), S));
    RC_TRY(load_N(g.c, od));
    RC_TRY(harc_amd_encode(g.c));
    RC_TRY(write_stage2(g.c, od));
    harc_amd_counters C; harc_amd_get_counters(g.c, &C);
    printf("Encoding done:\n%llu singleton reads were aligned\n%llu reads with N were aligned\n",        // encoder.cpp:506-508
           (unsigned long long)C.aligned_singletons, (unsigned long long)C.aligned_N);
    return HARC_AMD_OK;
}

extern "C" int harc_amd_compress_files(const harc_amd_params *params, const char *basedir)
{
    if (!params || !basedir) return HARC_AMD_EINVAL;
    CtxGuard g; RC_TRY(harc_amd_create(params, &g.c));
    const std::string od = std::string(basedir) + "/output/";
    RC_TRY(load_clean(g.c, od));
    RC_TRY(load_N(g.c, od));
    RC_TRY(harc_amd_reorder(g.c));
    RC_TRY(harc_amd_encode(g.c));
    RC_TRY(spit_stream(g.c, HARC_AMD_S1_ORDER_SINGLETON, 0, od + "read_order.bin.singleton"));          // harc:133 removes *.singleton
    RC_TRY(write_stage2(g.c, od));
    harc_amd_counters C; harc_amd_get_counters(g.c, &C);
    printf("Reordering done, %llu were unmatched\n", (unsigned long long)C.unmatched);
    printf("Encoding done:\n%llu singleton reads were aligned\n%llu reads with N were aligned\n",
           (unsigned long long)C.aligned_singletons, (unsigned long long)C.aligned_N);
    return HARC_AMD_OK;
}

extern "C" int harc_amd_pack_order_files(const harc_amd_params *params, const char *basedir)
{
    if (!params || !basedir) return HARC_AMD_EINVAL;
    CtxGuard g; RC_TRY(harc_amd_create(params, &g.c));
    const std::string od = std::string(basedir) + "/output/";
    std::vector<char> in;
    if (!slurp_file(od + "read_order.bin", in, true)) return HARC_AMD_EIO;
    std::vector<uint8_t> &b = out_buf(g.c, HARC_AMD_S2_ORDER, 0);
    b.assign(in.begin(), in.end());
    g.c->have_s2 = true;
    RC_TRY(harc_amd_pack_order(g.c));
    RC_TRY(spit_stream(g.c, HARC_AMD_P_ORDER, 0, od + "read_order.bin"));
    RC_TRY(spit_stream(g.c, HARC_AMD_P_ORDER_TAIL, 0, od + "read_order.bin.tail"));
    return HARC_AMD_OK;
}

// preprocess.out <fastq> <basedir> <preserve_order> <preserve_quality> <readlen>   (src/preprocess.cpp:50-137)
// Splits the FASTQ into output/input_clean.dna (reads without N), output/input_N.dna, output/read_order_N.bin and
// output/numreads.bin.  Quality / id side files (-q) are outside the hot path and not produced here.
extern "C" int harc_amd_preprocess_files(const char *fastq, const char *basedir, int32_t readlen)
{
    if (!fastq || !basedir || readlen < 1 || readlen > 255) { harc_set_error("preprocess: bad arguments"); return HARC_AMD_EINVAL; }
    FILE *in = fopen(fastq, "rb");
    if (!in) { harc_set_error("cannot open %s", fastq); return HARC_AMD_EIO; }
    const std::string od = std::string(basedir) + "/output/";
    FILE *fc = fopen((od + "input_clean.dna").c_str(), "wb"), *fn = fopen((od + "input_N.dna").c_str(), "wb"),
         *fo = fopen((od + "read_order_N.bin").c_str(), "wb");
    if (!fc || !fn || !fo) { if (fc) fclose(fc); if (fn) fclose(fn); if (fo) fclose(fo); fclose(in); harc_set_error("cannot create files under %s", od.c_str()); return HARC_AMD_EIO; }
    std::vector<char> buf(1 << 16);
    std::string line;
    uint64_t readnum = 0, nclean = 0; int li = 0, rc = HARC_AMD_OK;
    auto flush_line = [&]() {
        if (li == 1) {
            if ((int)line.size() != readlen) {                    // preprocess.cpp:92-97
                printf("Read length not fixed. Found two different read lengths: %d and %zu\n", readlen, line.size());
                harc_set_error("read length not fixed"); rc = HARC_AMD_EINVAL; return;
            }
            if (line.find('N') != std::string::npos) {
                fwrite(line.data(), 1, line.size(), fn); fputc('\n', fn);
                const uint32_t rn = (uint32_t)readnum; fwrite(&rn, 4, 1, fo);          // low 4 bytes of the counter, preprocess.cpp:102
            } else { fwrite(line.data(), 1, line.size(), fc); fputc('\n', fc); nclean++; }
        }
        if (li == 3) readnum++;
        li = (li + 1) & 3;
        line.clear();
    };
    size_t got;
    while (rc == HARC_AMD_OK && (got = fread(buf.data(), 1, buf.size(), in)) > 0) {
        size_t s = 0;
        for (size_t i = 0; i < got && rc == HARC_AMD_OK; i++)
            if (buf[i] == '\n') { line.append(buf.data() + s, i - s); s = i + 1; flush_line(); }
        if (s < got) line.append(buf.data() + s, got - s);
    }
    if (rc == HARC_AMD_OK && !line.empty()) flush_line();
    fclose(in); fclose(fc); fclose(fn); fclose(fo);
    if (rc != HARC_AMD_OK) return rc;
    if (readnum > 4294967290ull) { printf("Too many reads. HARC supports at most 4294967290 reads\n"); harc_set_error("too many reads"); return HARC_AMD_EINVAL; }   // :122-126
    const uint32_t n32 = (uint32_t)nclean;
    RC_TRY(spit_file(od + "numreads.bin", &n32, 4));
    printf("Read length: %d\nTotal number of reads: %llu\nTotal number of reads without N: %llu\nPreprocessing Done!\n", readlen,
           (unsigned long long)readnum, (unsigned long long)nclean);
    return HARC_AMD_OK;
}

// ------------------------------------------------------------------------------------------------ multi-GPU: merge of the rank parts
// Every rank of harc_amd_compress_fastq_shard_files leaves, under <basedir>/output/.shard/, its part of the files that exist once per
// archive.  The layout the decoders expect (encoder.cpp:457-503, decoder.cpp:141-169, decoder_preserve.cpp:212-290):
//   read_order.bin       = [aligned clean reads, shard by shard][unaligned singletons in read_singleton.txt order]
//   read_order_N_pe.bin  = [aligned N reads, shard by shard][unaligned N reads in input_N.dna order]
// so the aligned halves of all ranks come first, in rank order (= shard order rank*E + e), then the unaligned halves in rank order,
// and read_singleton.txt / input_N.dna are the rank parts in the same rank order.  read_singleton.txt packs 4 bases per byte
// (encoder.cpp:527-548) with up to 3 bases of ASCII tail: the parts are re-packed across the joints.
namespace {
struct Appender {
    FILE *f = nullptr; std::string path;
    int open(const std::string &p) { path = p; f = fopen(p.c_str(), "wb"); if (!f) { harc_set_error("cannot create %s", p.c_str()); return HARC_AMD_EIO; } return HARC_AMD_OK; }
    int add(const void *p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { harc_set_error("short write on %s", path.c_str()); return HARC_AMD_EIO; } return HARC_AMD_OK; }
    int add_file(const std::string &src, bool must_exist)
    {
        FILE *in = fopen(src.c_str(), "rb");
        if (!in) { if (must_exist) { harc_set_error("cannot open %s", src.c_str()); return HARC_AMD_EIO; } return HARC_AMD_OK; }
        std::vector<char> buf((size_t)4 << 20); size_t got; int rc = HARC_AMD_OK;
        while (rc == HARC_AMD_OK && (got = fread(buf.data(), 1, buf.size(), in)) > 0) rc = add(buf.data(), got);
        fclose(in);
        return rc;
    }
    ~Appender() { if (f) fclose(f); }
};
}

extern "C" int harc_amd_merge_shard_files(const char *basedir, int32_t world)
{
    if (!basedir || world < 1) { harc_set_error("merge_shard_files: bad arguments"); return HARC_AMD_EINVAL; }
    const std::string od = std::string(basedir) + "/output/", sd = od + ".shard/";
    auto part = [&](const char *stem, int r) { return sd + stem + "." + std::to_string(r); };
    // totals (and the proof that every rank finished)
    int L = 0; unsigned long long nrec = 0, nclean = 0, unmatched = 0, al_s = 0, al_N = 0;
    for (int r = 0; r < world; r++) {
        std::vector<char> st;
        if (!slurp_file(part("stats", r), st, true)) { harc_set_error("rank %d left no result under %s", r, sd.c_str()); return HARC_AMD_EIO; }
        st.push_back(0);
        int l = 0; unsigned long long v[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        if (sscanf(st.data(), "%d %llu %llu %llu %llu %llu %llu %llu %llu", &l, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7]) != 9) { harc_set_error("stats of rank %d unreadable", r); return HARC_AMD_EIO; }
        if (r && l != L) { harc_set_error("ranks disagree on the read length (%d vs %d)", L, l); return HARC_AMD_EINVAL; }
        L = l; nrec += v[0]; nclean += v[1]; unmatched += v[3]; al_s += v[4]; al_N += v[5];
    }
    if (nrec > 4294967290ull) { printf("Too many reads. HARC supports at most 4294967290 reads\n"); harc_set_error("too many reads"); return HARC_AMD_EINVAL; }
    printf("Read length: %d\nTotal number of reads: %llu\nTotal number of reads without N: %llu\nPreprocessing Done!\n", L, nrec, nclean);   // preprocess.cpp:133-136
    printf("Reordering done, %llu were unmatched\n", unmatched);                                                    // reorder.cpp:701
    printf("Encoding done:\n%llu singleton reads were aligned\n%llu reads with N were aligned\n", al_s, al_N);      // encoder.cpp:506-508
    {
        Appender o, on, in_n, oN;
        RC_TRY(o.open(od + "read_order.bin")); RC_TRY(on.open(od + "read_order_N_pe.bin")); RC_TRY(in_n.open(od + "input_N.dna")); RC_TRY(oN.open(od + "read_order_N.bin"));
        for (int r = 0; r < world; r++) { RC_TRY(o.add_file(part("order_a", r), true)); RC_TRY(on.add_file(part("orderN_a", r), true)); }
        for (int r = 0; r < world; r++) {
            RC_TRY(o.add_file(part("order_u", r), true)); RC_TRY(on.add_file(part("orderN_u", r), true));
            RC_TRY(in_n.add_file(part("input_N", r), true)); RC_TRY(oN.add_file(part("order_N", r), true));
        }
    }
    {   // read_singleton.txt: 2 bits per base across the joints (A0 C1 G2 T3, first base in the low bits: encoder.cpp:540-541)
        Appender sg; RC_TRY(sg.open(od + "read_singleton.txt"));
        unsigned pend = 0; int npend = 0;                          // bases waiting for a full byte
        std::vector<char> in, tail; std::vector<uint8_t> outb;
        auto code = [](char ch) -> unsigned { return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : 3u; };
        for (int r = 0; r < world; r++) {
            if (!slurp_file(part("singleton", r), in, true) || !slurp_file(part("singleton_tail", r), tail, true)) return HARC_AMD_EIO;
            if (npend == 0) RC_TRY(sg.add(in.data(), in.size()));
            else {
                outb.resize(in.size());
                const int sh = 2 * npend;
                for (size_t i = 0; i < in.size(); i++) { const unsigned b = (uint8_t)in[i]; outb[i] = (uint8_t)(pend | (b << sh)); pend = b >> (8 - sh); }
                RC_TRY(sg.add(outb.data(), outb.size()));
            }
            for (char ch : tail) {
                pend |= code(ch) << (2 * npend);
                if (++npend == 4) { const uint8_t b = (uint8_t)pend; RC_TRY(sg.add(&b, 1)); pend = 0; npend = 0; }
            }
        }
        char t[4]; for (int k = 0; k < npend; k++) t[k] = "ACGT"[(pend >> (2 * k)) & 3];
        RC_TRY(spit_file(od + "read_singleton.txt.tail", t, (size_t)npend));
    }
    { const uint32_t n32 = (uint32_t)nclean; RC_TRY(spit_file(od + "numreads.bin", &n32, 4)); }
    { char m[32]; const int ml = snprintf(m, sizeof m, "%d\n", L); RC_TRY(spit_file(od + "read_meta.txt", m, (size_t)ml)); }
    {   // -q -p: quality values and ids in file order = the slices in rank order
        FILE *probe = fopen(part("quality", 0).c_str(), "rb");
        if (probe) {
            fclose(probe);
            Appender q, i; RC_TRY(q.open(od + "output.quality")); RC_TRY(i.open(od + "output.id"));
            for (int r = 0; r < world; r++) { RC_TRY(q.add_file(part("quality", r), true)); RC_TRY(i.add_file(part("id", r), true)); }
        }
    }
    // the parts are gone from the archive
    static const char *stems[] = { "stats", "order_a", "order_u", "orderN_a", "orderN_u", "input_N", "order_N", "singleton", "singleton_tail", "quality", "id" };
    for (int r = 0; r < world; r++) for (const char *s : stems) (void)remove(part(s, r).c_str());
    (void)remove((sd + "comm_id").c_str());
    (void)remove(sd.substr(0, sd.size() - 1).c_str());            // rmdir when empty (a mailbox directory, if any, is the caller's)
    return HARC_AMD_OK;
}
