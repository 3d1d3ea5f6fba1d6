// motif_host_check.cpp -- the list parser and the host twin of the match by sequence (harc_amd/csrc/motif.h) under a sanitizer, as a program of its own; no device,
// no library.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I harc_amd/csrc tools/motif_host_check.cpp -o /tmp/motif_host_check
//   python -c "import sys, struct; from tests import match_cases as mc; o = open(sys.argv[1], 'wb'); [o.write(struct.pack('<IIQQ', c['k'], c['L'], len(c['motifs']), len(c['reads'])) + c['motifs'] + mc.text_of(c['reads']) + c['flags'] + c['hits'] + bytes(1024 - len(c['hits']))) for c in mc.cases().values()]; [o.write(struct.pack('<IIQQ', k, 0, len(t), 0) + t + bytes(1024)) for t, k, line in mc.refusals()]" /tmp/motif.cases
//   /tmp/motif_host_check /tmp/motif.cases
// The file holds, per case, K, the read length, the bytes of the list and the number of reads, then the list, the reads as lines of L + 1, the flags expected and 1024
// bytes of hits expected.  A case of read length 0 is a list that the rule must refuse.  Every text is copied into a heap block of exactly its size, so that a read or
// a write one byte outside it is reported; the flags and hits are written into blocks of exactly their size too.  The table of the device is built for every list
// that is taken and held against the motifs: the planes must spell the motif and its reverse complement.
#include <stdio.h>
#include <stdlib.h>
#include "motif.h"

static uint8_t *block(FILE *f, uint64_t n)
{
    uint8_t *p = (uint8_t *)malloc(n ? (size_t)n : 1);
    if (n && fread(p, 1, (size_t)n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return p;
}
// the sequence that an entry's planes spell
static std::string spelled(const MtEntry &e)
{
    std::string s(e.m, '?');
    for (uint32_t j = 0; j < e.m; j++) {
        const uint32_t lo = (e.w[j >> 5][MT_LO] >> (j & 31)) & 1u, hi = (e.w[j >> 5][MT_HI] >> (j & 31)) & 1u, care = (e.w[j >> 5][MT_CARE] >> (j & 31)) & 1u;
        for (const char b : { 'A', 'C', 'G', 'T' }) if (care && mt_lo((uint8_t)b) == lo && mt_hi((uint8_t)b) == hi) s[j] = b;
        if (!care) s[j] = (lo | hi) ? '!' : 'N';
    }
    return s;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s <cases>\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    struct { uint32_t K, L; uint64_t list_bytes, reads; } h;
    uint64_t cases = 0, refused = 0, reads = 0, selected = 0, entries = 0;
    while (fread(&h, sizeof h, 1, f) == 1) {
        uint8_t *list = block(f, h.list_bytes);
        std::vector<std::string> motifs; std::string why;
        const bool ok = mt_parse(list, h.list_bytes, h.K, &motifs, &why);
        if (h.L == 0) {
            uint8_t *skip = block(f, 1024);
            if (ok) { fprintf(stderr, "case %llu: a list that the rule refuses was taken\n", (unsigned long long)cases); return 1; }
            refused++; cases++;
            free(skip); free(list);
            continue;
        }
        if (!ok) { fprintf(stderr, "case %llu: the list was refused: %s\n", (unsigned long long)cases, why.c_str()); return 1; }
        const std::vector<MtEntry> tab = mt_table(motifs);
        for (size_t k = 0; k < motifs.size(); k++)
            if (spelled(tab[2 * k]) != motifs[k] || spelled(tab[2 * k + 1]) != mt_rc(motifs[k]) || tab[2 * k].owner != k || tab[2 * k + 1].owner != k) {
                fprintf(stderr, "case %llu: the planes of motif %zu do not spell it\n", (unsigned long long)cases, k); return 1; }
        entries += tab.size();
        const uint64_t S = (uint64_t)h.L + 1;
        uint8_t *dna = block(f, h.reads * S), *want = block(f, h.reads), *want_hit = block(f, 1024);
        uint8_t *flags = (uint8_t *)malloc(h.reads ? (size_t)h.reads : 1), *hit = (uint8_t *)calloc(motifs.size(), 1);
        selected += mt_flags_host(motifs, h.K, dna, h.reads, h.L, flags, hit);
        if (memcmp(flags, want, (size_t)h.reads) != 0 || memcmp(hit, want_hit, motifs.size()) != 0) { fprintf(stderr, "case %llu: flags or hits differ from the expected ones\n", (unsigned long long)cases); return 1; }
        reads += h.reads; cases++;
        free(list); free(dna); free(want); free(want_hit); free(flags); free(hit);
    }
    fclose(f);
    printf("%llu cases, %llu of them lists refused, %llu table entries spelled back, %llu reads, %llu selected: ok\n", (unsigned long long)cases, (unsigned long long)refused,
           (unsigned long long)entries, (unsigned long long)reads, (unsigned long long)selected);
    return cases && refused && selected ? 0 : 1;
}
