"""BGZF output without a GPU: the member encoder of harc_amd/csrc/deflate_member.h (the source the deflate kernel compiles) built for the host with g++,
AddressSanitizer and UBSan as a stand-alone program, together with the decoder of inflate_member.h.  What it writes is read back by Python's zlib and by
im_member; its code-length routine is called directly with counts that force the length limit; its tokens are checked against the token rule."""
import gzip
import heapq
import os
import random
import shutil
import struct
import subprocess
import zlib

import pytest

from tests import bgzf_out_cases as cases
from tests import bgzf_util as bu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = bytes.fromhex("1f8b08040000000000ff0600424302 00".replace(" ", ""))          # 16 bytes, then BSIZE

DRIVER = r"""
#include "deflate_member.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
// enc: cases [u32 n][n bytes] -> [u32 status][u32 bytes][the members, one per 65 280 bytes of text, no marker].  Every buffer is a heap block of exactly its
// size: a read or write past it is an AddressSanitizer report.  status: 1 a second run into a block of the member's exact size differs, 2 im_member does not
// return the text, 4 the tokens do not reproduce the text, 8 a token breaks its bounds
// len: cases [u32 n][u32 limit][n x u32 counts] -> [n bytes of code lengths]
static uint32_t one_member(const uint8_t *text, uint32_t n, const uint32_t *crc, FILE *o, uint32_t *total)
{
    uint32_t st = 0;
    DmHost *H = (DmHost *)malloc(sizeof(DmHost));
    uint8_t *big = (uint8_t *)malloc(DM_MEMBER_MAX);
    const uint32_t size = dm_member(text, n, big, *H, crc);
    uint8_t *exact = (uint8_t *)malloc(size);
    if (dm_member(text, n, exact, *H, crc) != size || memcmp(big, exact, size)) st |= 1;
    uint8_t *back = (uint8_t *)malloc(n);
    ImTables *t = (ImTables *)malloc(sizeof(ImTables));
    uint32_t mb = 0, tb = 0;
    if (im_member(exact, size, back, n, *t, crc, &mb, &tb) != IM_OK || mb != size || tb != n || memcmp(back, text, n)) st |= 2;
    // the tokens: literals and (length, distance) that rebuild the text from inside the member
    uint8_t *re = (uint8_t *)malloc(n);
    uint32_t at = 0;
    for (uint32_t i = 0; i < H->ntok && !(st & 8); i++) {
        const uint32_t k = H->tok[i];
        if (!(k >> 31)) { if (at >= n) st |= 8; else re[at++] = (uint8_t)k; continue; }
        const uint32_t len = dm_tok_len(k), d = dm_tok_dist(k);
        if (len < 3 || len > 258 || d < 1 || d > 32768 || d > at || len > n - at) { st |= 8; break; }
        for (uint32_t q = 0; q < len; q++) re[at + q] = re[at + q - d];
        at += len;
    }
    if (!(st & 8) && (at != n || memcmp(re, text, n))) st |= 4;
    fwrite(exact, 1, size, o); *total += size;
    free(re); free(t); free(back); free(exact); free(big); free(H);
    return st;
}
int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    FILE *f = fopen(argv[2], "rb"), *o = fopen(argv[3], "wb");
    if (!f || !o) return 2;
    uint32_t crc[256];
    for (uint32_t i = 0; i < 256; i++) crc[i] = im_crc_entry(i);
    uint32_t n;
    if (!strcmp(argv[1], "len")) {
        while (fread(&n, 4, 1, f) == 1) {
            uint32_t limit;
            if (fread(&limit, 4, 1, f) != 1) return 3;
            uint32_t *freq = (uint32_t *)malloc(4 * n), *A = (uint32_t *)malloc(4 * n);
            uint16_t *srt = (uint16_t *)malloc(2 * n), *blc = (uint16_t *)malloc(2 * 16);
            uint8_t *len = (uint8_t *)malloc(n);
            if (fread(freq, 4, n, f) != n) return 3;
            dm_lengths(freq, (int)n, (int)limit, len, A, srt, blc);
            fwrite(len, 1, n, o);
            free(len); free(blc); free(srt); free(A); free(freq);
        }
    } else {
        while (fread(&n, 4, 1, f) == 1) {
            uint8_t *p = (uint8_t *)malloc(n ? n : 1);
            if (n && fread(p, 1, n, f) != n) return 3;
            uint32_t st = 0, total = 0;
            const long head = ftell(o);
            fwrite(&st, 4, 1, o); fwrite(&total, 4, 1, o);
            for (uint32_t a = 0; a < n; a += DM_TEXT) {
                const uint32_t m = n - a < DM_TEXT ? n - a : DM_TEXT;
                uint8_t *text = (uint8_t *)malloc(m);                  // the member's text alone: nothing in front of it may be read
                memcpy(text, p + a, m);
                st |= one_member(text, m, crc, o, &total);
                free(text);
            }
            fseek(o, head, SEEK_SET); fwrite(&st, 4, 1, o); fwrite(&total, 4, 1, o); fseek(o, 0, SEEK_END);
            free(p);
        }
    }
    fclose(o); fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the host form of deflate_member.h")
    d = tmp_path_factory.mktemp("dm")
    src = d / "drv.cpp"
    src.write_text(DRIVER)
    exe = d / "drv"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-Wall", "-Werror", "-I", os.path.join(ROOT, "harc_amd", "csrc"), str(src), "-o", str(exe)])

    def run(mode, blob):
        cin, cout = d / "in.bin", d / "out.bin"
        cin.write_bytes(blob)
        r = subprocess.run([str(exe), mode, str(cin), str(cout)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]                  # the sanitizers are silent
        return cout.read_bytes()
    return run


def _encode(driver, texts):
    out = driver("enc", b"".join(struct.pack("<I", len(t)) + t for t in texts))
    res, at = [], 0
    for _ in texts:
        st, n = struct.unpack_from("<II", out, at)
        res.append((st, out[at + 8:at + 8 + n]))
        at += 8 + n
    assert at == len(out)
    return res


def _check_members(text, blob):
    """the frame of every member, and zlib's reading of the whole"""
    ms = bu.members(blob) if blob else []
    assert len(ms) == (len(text) + cases.MEMBER - 1) // cases.MEMBER
    for i, (off, size) in enumerate(ms):
        assert blob[off:off + 16] == HEADER and struct.unpack_from("<H", blob, off + 16)[0] == size - 1
        assert size <= 65536
        crc, isize = struct.unpack_from("<II", blob, off + size - 8)
        want = text[i * cases.MEMBER:(i + 1) * cases.MEMBER]
        assert isize == len(want) <= 65280 and crc == zlib.crc32(want)
        assert zlib.decompress(blob[off + 18:off + size - 8], -15) == want
    assert (gzip.decompress(blob) if blob else b"") == text


def test_listed_texts_round_trip_through_zlib_and_im_member(driver):
    t = cases.texts()
    names = sorted(t)
    res = _encode(driver, [t[k] for k in names])
    for k, (st, blob) in zip(names, res):
        assert st == 0, (k, st)
        _check_members(t[k], blob)
    size = {k: len(b) for k, (_, b) in zip(names, res)}
    # what each text is there for
    assert size["random_70000"] == 70000 + 2 * 31                  # two stored members
    assert 65280 // 8 < size["one_symbol_member"] < 65280 // 8 + 100          # no line, no match: one bit per byte
    assert size["newlines_1000"] < 100                              # matches at distance 4 that overlap themselves
    assert size["identical_300_L255"] < 3000                        # runs far above 258, cut into pieces


def test_every_run_length_is_in_its_text():
    """the text meant to hold a run of every length 3 .. 258 holds them (runs that a member boundary cuts aside)"""
    text = cases.every_run_length()
    runs = set()
    for a in range(0, len(text), cases.MEMBER):
        runs |= set(cases.run_lengths(text[a:a + cases.MEMBER]))
    # the first records of every member have no line four back inside it: their lengths are made up by a second copy shifted by half a member
    shifted = text[cases.MEMBER // 2:]
    for a in range(0, len(shifted), cases.MEMBER):
        runs |= set(cases.run_lengths(shifted[a:a + cases.MEMBER]))
    assert set(range(3, 259)) <= runs, sorted(set(range(3, 259)) - runs)


def test_shifted_run_lengths_and_random_cuts_round_trip(driver):
    rng = random.Random(21)
    fq = bu.fastq_text(1500, 100, seed=9)
    fq255 = bu.fastq_text(300, 255, seed=5)
    texts = [cases.every_run_length()[cases.MEMBER // 2:]]
    for _ in range(300):
        src = fq if rng.random() < 0.8 else fq255
        n = rng.choice([rng.randrange(1, 600), rng.randrange(1, 20000), rng.randrange(60000, 70000)])
        a = rng.randrange(0, len(src) - n)
        texts.append(src[a:a + n])
    for text, (st, blob) in zip(texts, _encode(driver, texts)):
        assert st == 0, (len(text), st)
        _check_members(text, blob)


def _lengths(driver, vectors):
    blob = b"".join(struct.pack("<II", len(f), limit) + struct.pack("<%dI" % len(f), *f) for f, limit in vectors)
    out = driver("len", blob)
    res, at = [], 0
    for f, _ in vectors:
        res.append(list(out[at:at + len(f)]))
        at += len(f)
    assert at == len(out)
    return res


def test_code_lengths_respect_the_limit_and_fill_the_code_space(driver):
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    rng = random.Random(2)
    vectors = []
    for k in range(9, 20):                                         # the unlimited depth of k Fibonacci counts is k - 1 > 7
        vectors.append((fib[:k], 7))
        v = fib[:k] + [0] * (19 - k); rng.shuffle(v); vectors.append((v, 7))
    for k in range(17, 41):                                        # ... > 15
        vectors.append((fib[:k], 15))
        v = fib[:k] + [0] * (286 - k); rng.shuffle(v); vectors.append((v, 15))
    vectors.append(([0] * 100 + [5] + [0] * 185, 15))              # a single symbol: one code of one bit
    vectors.append(([0] * 7 + [3], 7))
    vectors.append(([9, 0, 0, 1], 15))                             # two symbols
    vectors.append(([1] * 286, 15))                                # all equal
    vectors.append(([1] * 19, 7))
    vectors.append(([0] * 30, 15))                                 # none
    for _ in range(200):
        n = rng.choice([19, 30, 286])
        vectors.append(([rng.choice([0, 0, 1, 2, 3, 10, 100, 1000, 60000]) if rng.random() < 0.7 else rng.randrange(1, 65000) for _ in range(n)], 7 if n == 19 else 15))
    for (freq, limit), lens in zip(vectors, _lengths(driver, vectors)):
        used = [l for f, l in zip(freq, lens) if f]
        assert all(l == 0 for f, l in zip(freq, lens) if not f)
        assert all(1 <= l <= limit for l in used), (freq, lens)      # no symbol with a count is left without a code
        kraft = sum(2 ** (limit - l) for l in used)
        if len(used) == 1:
            assert used == [1]                                     # the one-code case RFC 1951 allows
        elif used:
            assert kraft == 2 ** limit, (freq, lens)
        # not worse than a code of fixed width, and optimal where the limit does not bind
        cost = sum(f * l for f, l in zip(freq, lens))
        if len(used) > 1:
            h = [(f, i) for i, f in enumerate(freq) if f]
            heapq.heapify(h); opt, nid = 0, len(freq)
            while len(h) > 1:
                a, b = heapq.heappop(h), heapq.heappop(h)
                opt += a[0] + b[0]; nid += 1
                heapq.heappush(h, (a[0] + b[0], nid))
            assert cost >= opt
            if max(used) < limit:
                assert cost == opt, (freq, lens)


def test_library_host_encoder_and_bound_without_a_device():
    """the encoder in a row behind the C-ABI (what the GPU test holds the kernels to) and harc_amd_bgzf_bound: no device is touched"""
    import harc_amd
    assert [harc_amd.bgzf_bound(n) for n in (0, 1, 65280, 65281)] == [28, 65311 + 28, 65311 + 28, 2 * 65311 + 28]
    t = cases.texts()
    for k in ("empty", "one_byte", "fastq_cut_130561", "random_70000", "every_run_length_L255"):
        blob = harc_amd.bgzf_deflate_host(t[k])
        assert blob.endswith(bu.EOF_MARKER) and len(blob) <= harc_amd.bgzf_bound(len(t[k]))
        _check_members(t[k], blob[:-28])
        assert harc_amd.bgzf_deflate_host(t[k], eof=False) == blob[:-28]
