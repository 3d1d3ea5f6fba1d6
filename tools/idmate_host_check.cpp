// idmate_host_check.cpp -- the host twins of the mate rule (harc_amd/csrc/idmate.h) under a sanitizer, as a program of its own; no device, no library.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I harc_amd/csrc tools/idmate_host_check.cpp -o /tmp/idmate_host_check
//   python -c "import sys, struct; from tests import idmate_cases as mc; o = open(sys.argv[1], 'wb'); [o.write(struct.pack('<QQ', len(a), len(b)) + a + b) for a, b in mc.cases().values()]" /tmp/idmate.cases
//   /tmp/idmate_host_check /tmp/idmate.cases
// The file holds, per case, two u64 lengths and the two id texts.  Every text is copied into a heap block of exactly its size, so that a read or a write one byte
// outside it is reported; the rule is found, and the first text is patched by every rule.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "idmate.h"

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s <cases>\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint64_t len[2], cases = 0, lines = 0, bad = 0; uint32_t seen = 0;
    while (fread(len, 8, 2, f) == 2) {
        uint8_t *t[2];
        for (int k = 0; k < 2; k++) {
            t[k] = (uint8_t *)malloc(len[k] ? (size_t)len[k] : 1);
            if (len[k] && fread(t[k], 1, (size_t)len[k], f) != len[k]) { fprintf(stderr, "short case file\n"); return 2; }
        }
        uint64_t la = 0, lb = 0; int oa = 0, ob = 0;
        idm_count_lines_host(t[0], len[0], &la, &oa); idm_count_lines_host(t[1], len[1], &lb, &ob);
        if (la != lb || oa || ob) { fprintf(stderr, "case %llu: the texts are not closed lines of one count\n", (unsigned long long)cases); return 1; }
        const uint32_t flags = idm_rule_flags_host(t[0], len[0], t[1], len[1]);
        const int32_t rule = idm_rule_of(flags, la);
        seen |= 1u << rule;
        for (int32_t r = IDM_NONE; r <= IDM_SPACE; r++) {
            uint8_t *w = (uint8_t *)malloc(len[0] ? (size_t)len[0] : 1);
            memcpy(w, t[0], (size_t)len[0]);
            const uint64_t b = idm_apply_host(w, len[0], r);
            if (r == rule && r != IDM_NONE && (b != 0 || memcmp(w, t[1], (size_t)len[0]) != 0)) { fprintf(stderr, "case %llu: apply(A, %s) != B\n", (unsigned long long)cases, idm_rule_name(r)); return 1; }
            bad += b;
            free(w);
        }
        cases++; lines += la;
        free(t[0]); free(t[1]);
    }
    fclose(f);
    printf("%llu cases, %llu pairs of lines, rules seen 0x%x, %llu lines refused by a rule that is not theirs: ok\n", (unsigned long long)cases, (unsigned long long)lines, seen, (unsigned long long)bad);
    return seen == 0xF ? 0 : 1;
}
