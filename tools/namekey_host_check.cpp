// namekey_host_check.cpp -- the host twins of the selection by name (harc_amd/csrc/namekey.h) under a sanitizer, as a program of its own; no device, no library.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I harc_amd/csrc tools/namekey_host_check.cpp -o /tmp/namekey_host_check
//   /tmp/namekey_host_check
// The lines and lists are generated here: names that end at every offset from 0 to 19 and from 60 to 69 and at 127 .. 129 and 300 (both sides of a lane's eight
// bytes and of a group's 64-byte step), ended by a space, a tab and the line's end, with and without '@', "/1" and "/2"; lists with duplicates, empty lines and
// comments; texts with and without the newline of their last line.  Every line and text is copied into a heap block of exactly its size, so that a read one byte
// outside it is reported.  The name of every line is held to a model written on std::string, the flags, counts and gathers to a std::set of the model's names,
// with all 64, 8 and 1 bits of the hash kept (with one bit every name shares a slot chain: the byte comparison and the probing decide).
#include <stdio.h>
#include <stdlib.h>
#include <set>
#include <string>
#include <vector>
#include "namekey.h"

static std::string model_key(const std::string &line)
{
    std::string s = (!line.empty() && line[0] == '@') ? line.substr(1) : line;
    const size_t e = s.find_first_of(" \t");
    if (e != std::string::npos) s.resize(e);
    if (s.size() >= 3 && s[s.size() - 2] == '/' && (s.back() == '1' || s.back() == '2')) s.resize(s.size() - 2);
    return s;
}
static std::string name_of(size_t n, unsigned salt)
{
    std::string s(n, 'A');
    for (size_t i = 0; i < n; i++) s[i] = (char)('A' + (7 * i + 3 * salt + n) % 26);
    return s;
}
// a copy in a heap block of exactly the text's size
struct Exact {
    uint8_t *p; uint64_t n;
    explicit Exact(const std::string &s) : p((uint8_t *)malloc(s.size() ? s.size() : 1)), n(s.size()) { if (n) memcpy(p, s.data(), (size_t)n); }
    ~Exact() { free(p); }
};
static std::string join(const std::vector<std::string> &ls, bool open)
{
    std::string t;
    for (const std::string &l : ls) { t += l; t += '\n'; }
    if (open && !t.empty()) t.pop_back();
    return t;
}
static std::vector<std::string> split(const std::string &t)
{
    std::vector<std::string> out;
    size_t i = 0;
    while (i < t.size()) { size_t e = t.find('\n', i); if (e == std::string::npos) e = t.size(); out.push_back(t.substr(i, e - i)); i = e + 1; }
    return out;
}

int main()
{
    std::vector<size_t> lens;
    for (size_t n = 0; n <= 19; n++) lens.push_back(n);
    for (size_t n = 60; n <= 69; n++) lens.push_back(n);
    for (size_t n : { (size_t)127, (size_t)128, (size_t)129, (size_t)300 }) lens.push_back(n);
    std::vector<std::string> ids;
    for (size_t n : lens)
        for (const char *at : { "@", "" })
            for (const char *tail : { "", "/1", "/2" })
                for (const char *end : { "", " comment", "\tx" }) ids.push_back(std::string(at) + name_of(n, 0) + tail + end);
    for (const char *l : { "/1", "a/1", "ab/3", "a/1/2", "@a/1/2\tq", "r7", "r70", "@r7/1 comment", "r7/2", "@r7", "r7 x", "", "@", " ", "@ x", "a\r", "a/1\r", "//1", "@@x" }) ids.push_back(l);
    unsigned long long keys = 0, texts = 0, gathers = 0;
    for (const std::string &l : ids) {
        const Exact e(l);
        uint64_t off = 99, len = 99;
        nk_key(e.p, e.n, &off, &len);
        const std::string want = model_key(l);
        if (len != want.size() || off != ((!l.empty() && l[0] == '@') ? 1u : 0u) || l.compare((size_t)off, (size_t)len, want) != 0) { fprintf(stderr, "the name of '%s' is '%s', the twin says %llu + %llu\n", l.c_str(), want.c_str(), (unsigned long long)off, (unsigned long long)len); return 1; }
        if (nk_hash(e.p + off, len) != nk_hash((const uint8_t *)want.data(), want.size())) { fprintf(stderr, "the hash of '%s' depends on where the name lies\n", l.c_str()); return 1; }
        keys++;
    }
    std::vector<std::vector<std::string>> lists;
    { std::vector<std::string> a; for (size_t i = 0; i < ids.size(); i += 3) a.push_back(model_key(ids[i])); lists.push_back(a); }
    lists.push_back({ "r7 first", "", "@r7/2", "r7", " ", "@", name_of(8, 0) + "\tc", "@" + name_of(8, 0) + "/1", "absent", "absent", name_of(300, 0) + " x" });
    lists.push_back({ "nobody" });
    lists.push_back({ "", "@", " " });
    { std::vector<std::string> a; for (const std::string &l : ids) a.push_back(l); lists.push_back(a); }
    for (const std::vector<std::string> &list : lists)
        for (int open_list = 0; open_list < 2; open_list++)
            for (int open_ids = 0; open_ids < 2; open_ids++) {
                std::vector<std::string> idl = ids;
                if (open_ids) idl.push_back("@" + name_of(65, 0) + "/2 last");      // (an open text cannot end in an empty line)
                const std::string nt = join(list, open_list != 0), it = join(idl, open_ids != 0);
                const Exact en(nt), ei(it);
                std::set<std::string> want_set;
                for (const std::string &l : split(nt)) if (!model_key(l).empty()) want_set.insert(model_key(l));
                const std::vector<std::string> il = split(it);
                std::vector<uint8_t> want(il.size());
                std::set<std::string> found;
                for (size_t i = 0; i < il.size(); i++) { const std::string k = model_key(il[i]); want[i] = want_set.count(k) ? 1 : 0; if (want[i]) found.insert(k); }
                for (uint32_t bits : { 64u, 8u, 1u }) {
                    uint8_t *flags = (uint8_t *)malloc(il.size() ? il.size() : 1);
                    uint64_t out[3] = { 0, 0, 0 };
                    nk_select_flags_host(en.p, en.n, ei.p, ei.n, bits, flags, out);
                    bool ok = out[0] == il.size() && out[1] == want_set.size() && out[2] == found.size();
                    for (size_t i = 0; ok && i < il.size(); i++) ok = flags[i] == want[i];
                    free(flags);
                    if (!ok) { fprintf(stderr, "list %zu (open %d), ids open %d, %u bits: the twin gives %llu lines, %llu names, %llu found; the model %zu, %zu, %zu, or other flags\n", (size_t)(&list - &lists[0]), open_list, open_ids, bits,
                                       (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2], il.size(), want_set.size(), found.size()); return 1; }
                    texts++;
                }
                if (nk_count_lines_host(ei.p, ei.n) != il.size()) { fprintf(stderr, "the twin counts other lines\n"); return 1; }
                // the gather of lines of any length, into a block of exactly the result's size
                std::string wg;
                for (size_t i = 0; i < il.size(); i++) if (want[i]) { wg += il[i]; if (i + 1 < il.size() || !open_ids) wg += '\n'; }
                const uint64_t need = nk_gather_host(ei.p, ei.n, 0, want.data(), want.size(), nullptr);
                uint8_t *g = (uint8_t *)malloc(need ? (size_t)need : 1);
                const uint64_t got = nk_gather_host(ei.p, ei.n, 0, want.data(), want.size(), g);
                const bool same = need == wg.size() && got == need && (!need || !memcmp(g, wg.data(), (size_t)need));
                free(g);
                if (!same) { fprintf(stderr, "the gather of the lines gives %llu bytes, the model %zu, or other bytes\n", (unsigned long long)got, wg.size()); return 1; }
                gathers++;
            }
    for (uint64_t stride : { (uint64_t)2, (uint64_t)101, (uint64_t)256 }) {
        const size_t n = 37;
        std::string t;
        for (size_t i = 0; i < n; i++) { for (uint64_t j = 0; j + 1 < stride; j++) t += (char)(0x21 + (i * 31 + j * 7) % 90); t += '\n'; }
        const Exact et(t);
        for (int pat = 0; pat < 5; pat++) {
            std::vector<uint8_t> f(n);
            for (size_t i = 0; i < n; i++) f[i] = pat == 0 ? 0 : pat == 1 ? 1 : pat == 2 ? i == 0 : pat == 3 ? i == n - 1 : (i * 5 % 7 < 3);
            std::string wg;
            for (size_t i = 0; i < n; i++) if (f[i]) wg += t.substr(i * (size_t)stride, (size_t)stride);
            uint8_t *g = (uint8_t *)malloc(wg.size() ? wg.size() : 1);
            const uint64_t got = nk_gather_host(et.p, et.n, stride, f.data(), n, g);
            const bool same = got == wg.size() && (!got || !memcmp(g, wg.data(), (size_t)got));
            free(g);
            if (!same) { fprintf(stderr, "the gather at stride %llu, pattern %d, gives other bytes\n", (unsigned long long)stride, pat); return 1; }
            gathers++;
        }
    }
    printf("%llu names, %llu pairs of texts at 64, 8 and 1 hash bits, %llu gathers: ok\n", keys, texts, gathers);
    return 0;
}
