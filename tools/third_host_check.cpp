// third_host_check.cpp -- the host twins of the rule of the third lines (harc_amd/csrc/third.h) under a sanitizer, as a program of its own; no device, no library.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I harc_amd/csrc tools/third_host_check.cpp -o /tmp/third_host_check
//   python -c "import sys, struct; from tests import third_cases as tc; o = open(sys.argv[1], 'wb'); [o.write(struct.pack('<QII', len(t), *tc.text_flags(t)) + t) for t in list(tc.cases().values()) + [tc.alignment_text(k) for k in range(41)]]" /tmp/third.cases
//   /tmp/third_host_check /tmp/third.cases
// The file holds, per case, a u64 length, the flag word and the record count the Python rule gives (u32 each), and the FASTQ text.  Every text is copied into a heap
// block of exactly its size, so that a read one byte outside it is reported; the text twin is run over it, and the line twin over every record found by a walk of
// its own, each line in a block of exactly its size.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "third.h"

static uint8_t *exact_copy(const uint8_t *p, uint64_t n)
{
    uint8_t *q = (uint8_t *)malloc(n ? (size_t)n : 1);
    if (n) memcpy(q, p, (size_t)n);
    return q;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s <cases>\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint64_t len = 0, cases = 0, records = 0; uint32_t want[2], seen = 0;
    while (fread(&len, 8, 1, f) == 1 && fread(want, 4, 2, f) == 2) {
        uint8_t *t = (uint8_t *)malloc(len ? (size_t)len : 1);
        if (len && fread(t, 1, (size_t)len, f) != len) { fprintf(stderr, "short case file\n"); return 2; }
        uint64_t n = 0;
        const uint32_t flags = th_text_flags_host(t, len, &n);
        if (flags != want[0] || n != want[1]) {
            fprintf(stderr, "case %llu: flags %u over %llu records, the Python rule gives %u over %u\n", (unsigned long long)cases, flags, (unsigned long long)n, want[0], want[1]);
            return 1;
        }
        // the line twin, record by record: lines found here, not by the twin under test
        std::vector<std::pair<uint64_t, uint64_t>> lines;
        for (uint64_t at = 0; at < len;) {
            uint64_t e = at;
            while (e < len && t[e] != '\n') e++;
            lines.emplace_back(at, e - at);
            at = e + 1;
        }
        uint32_t g = TH_F_ALL; uint64_t m = 0;
        for (size_t k = 2; k < lines.size(); k += 4) {
            uint8_t *a = exact_copy(t + lines[k - 2].first, lines[k - 2].second), *b = exact_copy(t + lines[k].first, lines[k].second);
            g &= th_record_flags_host(a, lines[k - 2].second, b, lines[k].second);
            m++;
            free(a); free(b);
        }
        if (g != flags || m != n) { fprintf(stderr, "case %llu: the line twin gives %u over %llu records, the text twin %u over %llu\n", (unsigned long long)cases, g, (unsigned long long)m, flags, (unsigned long long)n); return 1; }
        const int32_t rule = th_rule_of(flags, n);
        if (th_rule_parse(th_rule_name(rule)) != rule) { fprintf(stderr, "case %llu: the name of rule %d does not parse back\n", (unsigned long long)cases, (int)rule); return 1; }
        seen |= 1u << rule;
        cases++; records += n;
        free(t);
    }
    fclose(f);
    printf("%llu cases, %llu records, rules seen 0x%x: ok\n", (unsigned long long)cases, (unsigned long long)records, seen);
    return seen == 0x7 ? 0 : 1;
}
