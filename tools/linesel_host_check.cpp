// linesel_host_check.cpp -- the host twin of the line select (harc_amd/csrc/linesel.h) and its bit arithmetic under a sanitizer, as a program of its own; no
// device, no library.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I harc_amd/csrc tools/linesel_host_check.cpp -o /tmp/linesel_host_check
//   python -c "import sys, struct; from tests import range_cases as rc; o = open(sys.argv[1], 'wb'); [o.write(struct.pack('<Q', len(t)) + t) for t in rc.texts().values()]" /tmp/linesel.cases
//   /tmp/linesel_host_check /tmp/linesel.cases
// The file holds, per case, a u64 length and the text.  Every text is copied into a heap block of exactly its size, so that a read one byte outside it is
// reported.  Every line of every text is asked for, the answer is held to a byte loop, and the chunk arithmetic the kernels use (newline bits of a word, the
// bytes of a chunk that belong to the text, the n-th set bit) is run over the text at every alignment and held to the same loop.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "linesel.h"

// the text as the kernels see it: 16-byte chunks of a hull that starts `mis` bytes in front of the text -> the newline offsets, by the chunk arithmetic
static std::vector<uint64_t> by_chunks(const uint8_t *t, uint64_t n, uint64_t mis)
{
    std::vector<uint8_t> hull((size_t)((mis + n + 15) / 16 * 16), (uint8_t)'\n');      // newlines around the text: a byte that is counted by mistake shows
    if (n) memcpy(hull.data() + mis, t, (size_t)n);
    std::vector<uint64_t> at;
    for (uint64_t a = 0; a < hull.size(); a += 16) {
        uint32_t m = 0;
        for (int w = 0; w < 4; w++) { uint32_t x; memcpy(&x, hull.data() + a + 4 * w, 4); m |= ls_newline_bits(x) << (4 * w); }
        m &= ls_keep_bits(a, mis, mis + n);
        const uint32_t c = (uint32_t)__builtin_popcount(m);
        for (uint32_t r = 1; r <= c; r++) at.push_back(a + ls_nth_bit(m, r) - mis);
    }
    return at;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s <cases>\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint64_t len = 0, cases = 0, asked = 0;
    while (fread(&len, 8, 1, f) == 1) {
        uint8_t *t = (uint8_t *)malloc(len ? (size_t)len : 1);
        if (len && fread(t, 1, (size_t)len, f) != len) { fprintf(stderr, "short case file\n"); return 2; }
        std::vector<uint64_t> nl;
        for (uint64_t i = 0; i < len; i++) if (t[i] == '\n') nl.push_back(i);
        for (uint64_t k = 0; k <= nl.size() + 2; k++) {
            uint64_t out[2] = { 7, 7 };
            ls_line_offset_host(t, len, k, out);
            const uint64_t want = k == 0 ? 0 : k <= nl.size() ? nl[(size_t)k - 1] + 1 : LS_NONE;
            if (out[0] != nl.size() || out[1] != want) { fprintf(stderr, "case %llu: line %llu starts at %llu, the twin says %llu\n", (unsigned long long)cases, (unsigned long long)k, (unsigned long long)want, (unsigned long long)out[1]); return 1; }
            asked++;
        }
        for (uint64_t mis = 0; mis < 16; mis++)
            if (by_chunks(t, len, mis) != nl) { fprintf(stderr, "case %llu: the chunk arithmetic finds other newlines at alignment %llu\n", (unsigned long long)cases, (unsigned long long)mis); return 1; }
        free(t);
        cases++;
    }
    fclose(f);
    printf("%llu cases, %llu lines asked for, every alignment of the chunk arithmetic: ok\n", (unsigned long long)cases, (unsigned long long)asked);
    return cases ? 0 : 1;
}
