"""The packed quality file without a GPU: the block coder of harc_amd/csrc/qv_block.h (the source the kernels compile) built for the host with g++,
AddressSanitizer and UBSan as a stand-alone program; what the library's host twin writes read back by a decoder in plain Python written from the README's
format text; damaged files refused; the size against bz2 and xz; the bound and the empty file."""
import bz2
import lzma
import os
import random
import shutil
import struct
import subprocess

import pytest

from tests import quality_cases as qc
from tests.readme_decoders import quality_decode as readme_decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
MAGIC = b"HARCQ1\0\0"

DRIVER = r"""
#include "qv_block.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
// enc: cases [u32 n][u32 L][u32 rb][n * (L + 1) bytes] -> [u32 status][u32 bytes][the blocks, no file header].  Every buffer is a heap block of exactly its size:
// a read or write past it is an AddressSanitizer report.  status: 1 a second run into a block of the exact size differs, 2 qv_block_decode does not return the text
// dec: files [u32 bytes][the file] -> [u32 code][u32 block][u32 text bytes][text]; code 0, a QV_E_* of the first bad block, 100 a prefix that leaves the file, 101 the
// header.  The payload and the lines of every block are heap blocks of exactly their declared sizes
static uint32_t one_block(const uint8_t *lines, uint32_t m, uint32_t L, FILE *o, uint32_t *total)
{
    uint32_t st = 0;
    const size_t tb = (size_t)m * (L + 1);
    uint8_t *text = (uint8_t *)malloc(tb);                        // the block's lines alone
    memcpy(text, lines, tb);
    QvWork *W = (QvWork *)malloc(sizeof(QvWork));
    uint8_t *slabs = (uint8_t *)malloc(qv_block_slabs(m, L));
    uint8_t *big = (uint8_t *)malloc(5 + (size_t)m * L);
    int stored = 0;
    const uint32_t size = qv_block_encode(text, m, L, *W, slabs, big, 5 + (size_t)m * L, &stored);
    if (!size) return 4;
    uint8_t *exact = (uint8_t *)malloc(size);
    if (qv_block_encode(text, m, L, *W, slabs, exact, size, &stored) != size || memcmp(big, exact, size)) st |= 1;
    if (size > 1 && qv_block_encode(text, m, L, *W, slabs, exact, size - 1, &stored) != 0) st |= 1;
    uint8_t *payload = (uint8_t *)malloc(size - 4);
    memcpy(payload, exact + 4, size - 4);
    uint8_t *back = (uint8_t *)malloc(tb);
    if (qv_le32(exact) != size - 4 || qv_block_decode(payload, size - 4, m, L, *W, back) != QV_OK || memcmp(back, text, tb)) st |= 2;
    fwrite(exact, 1, size, o); *total += size;
    free(back); free(payload); free(exact); free(big); free(slabs); free(W); free(text);
    return st;
}
static uint32_t one_file(const uint8_t *f, uint32_t nbytes, FILE *o)
{
    uint32_t code = 0, tb = 0, block = 0;
    uint8_t *text = NULL;
    if (nbytes < 32 || !qv_magic_ok(f)) code = 101;
    else {
        const uint32_t L = qv_le32(f + 8), rb = qv_le32(f + 12); const uint64_t n = qv_le64(f + 16);
        if (n == 0) code = nbytes == 32 ? 0 : 101;
        else if (L < 1 || L > 255 || rb < 1 || n > 1000000) code = 101;
        else {
            tb = (uint32_t)(n * (L + 1));
            text = (uint8_t *)malloc(tb);
            memset(text, 0, tb);
            QvWork *W = (QvWork *)malloc(sizeof(QvWork));
            uint64_t at = 32;
            for (uint64_t a = 0; a < n; a += rb, block++) {
                const uint32_t m = n - a < rb ? (uint32_t)(n - a) : rb;
                if (nbytes - at < 4) { code = 100; break; }
                const uint32_t pb = qv_le32(f + at);
                if (pb == 0 || nbytes - at - 4 < pb) { code = 100; break; }
                uint8_t *payload = (uint8_t *)malloc(pb), *lines = (uint8_t *)malloc((size_t)m * (L + 1));
                memcpy(payload, f + at + 4, pb);
                memset(lines, 0, (size_t)m * (L + 1));
                code = (uint32_t)qv_block_decode(payload, pb, m, L, *W, lines);
                memcpy(text + a * (L + 1), lines, (size_t)m * (L + 1));
                free(lines); free(payload);
                if (code) break;
                at += 4 + (uint64_t)pb;
            }
            if (!code && at != nbytes) { code = 100; block--; }
            free(W);
        }
    }
    fwrite(&code, 4, 1, o); fwrite(&block, 4, 1, o); fwrite(&tb, 4, 1, o);
    if (tb) fwrite(text, 1, tb, o);
    free(text);
    return code;
}
int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    FILE *f = fopen(argv[2], "rb"), *o = fopen(argv[3], "wb");
    if (!f || !o) return 2;
    uint32_t n;
    if (!strcmp(argv[1], "dec")) {
        while (fread(&n, 4, 1, f) == 1) {
            uint8_t *p = (uint8_t *)malloc(n ? n : 1);
            if (n && fread(p, 1, n, f) != n) return 3;
            one_file(p, n, o);
            free(p);
        }
    } else {
        while (fread(&n, 4, 1, f) == 1) {
            uint32_t L, rb;
            if (fread(&L, 4, 1, f) != 1 || fread(&rb, 4, 1, f) != 1) return 3;
            const size_t tb = (size_t)n * (L + 1);
            uint8_t *p = (uint8_t *)malloc(tb ? tb : 1);
            if (tb && fread(p, 1, tb, f) != tb) return 3;
            if (!rb) rb = qv_default_rb(L);
            uint32_t st = 0, total = 0;
            const long head = ftell(o);
            fwrite(&st, 4, 1, o); fwrite(&total, 4, 1, o);
            for (uint32_t a = 0; a < n; a += rb) st |= one_block(p + (size_t)a * (L + 1), n - a < rb ? n - a : rb, L, o, &total);
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
        pytest.fail("g++ is needed to build the host form of qv_block.h")
    d = tmp_path_factory.mktemp("qv")
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


@pytest.fixture(scope="module")
def cases():
    return qc.small_cases()


def _default_rb(L):
    return max(256, (1 << 22) // L)


def _header(text, L, rb):
    n = len(text) // (L + 1)
    return MAGIC + (struct.pack("<IIQQ", L, rb or _default_rb(L), n, 0) if n else bytes(24))


def test_every_case_round_trips_in_the_sanitizer_build(driver, cases):
    names = sorted(cases)
    out = driver("enc", b"".join(struct.pack("<III", len(cases[k][0]) // (cases[k][1] + 1), cases[k][1], cases[k][2]) + cases[k][0] for k in names))
    import harc_amd
    at = 0
    for k in names:
        st, n = struct.unpack_from("<II", out, at)
        blocks, at = out[at + 8:at + 8 + n], at + 8 + n
        assert st == 0, (k, st)
        text, L, rb = cases[k]
        assert _header(text, L, rb) + blocks == harc_amd.qpack_host(text, L, rb), k      # the library's host twin is this code
    assert at == len(out)


def test_a_decoder_written_from_the_readme_reads_every_case(cases):
    import harc_amd
    sizes, modes = {}, {}
    for k, (text, L, rb) in sorted(cases.items()):
        f = harc_amd.qpack_host(text, L, rb)
        got, modes[k] = readme_decode(f)
        assert got == text, k
        assert harc_amd.qunpack_host(f) == text, k
        assert len(f) <= harc_amd.qpack_bound(len(text) // (L + 1), L, rb)
        sizes[k] = len(f)
    # what each case is there for
    assert modes["strands_1_L37"] == [0] and sizes["strands_1_L37"] == 32 + 5 + 37
    assert modes["byte_0x80_stored"] == [0]
    assert modes["middle_block_stored"] == [1, 0, 1]
    assert modes["one_symbol"] == [1] and sizes["one_symbol"] == 32 + 4 + 14 + 4 + 1024 + 4 * 256
    assert modes["cut_901_RB300"] == [1, 1, 1, 0] and modes["cut_300_RB300"] == [1] and modes["cut_301_RB300"] == [1, 0]
    assert modes["full_alphabet"] == [1] and sizes["full_alphabet"] < 600 * 255 * 0.96           # log2(94) / 8 = 0.82 of the text, and the table
    assert modes["dominant_symbol"] == [1] and sizes["dominant_symbol"] < 2300
    assert sizes["empty"] == 32


def test_corruption_is_refused(driver):
    import harc_amd
    text = qc.corruption_text()
    packed = harc_amd.qpack_host(text, 100)
    bad = qc.corrupted(packed)
    names = sorted(bad)
    out = driver("dec", b"".join(struct.pack("<I", len(bad[k])) + bad[k] for k in names))          # the sanitizer build reports nothing on any of them
    at, undetected = 0, 0
    for k in names:
        code, block, tb = struct.unpack_from("<III", out, at)
        got, at = out[at + 12:at + 12 + tb], at + 12 + tb
        try:
            back = harc_amd.qunpack_host(bad[k])
        except harc_amd.HarcAmdError as e:
            assert e.code == EINVAL and code != 0, (k, code, str(e))
            if not k.startswith(("wrong", "trunc")):
                assert "block 0 at byte 32" in str(e), (k, str(e))
            continue
        assert k.startswith("flip") and code == 0 and back == text and got == text, k          # a flip that decodes without an error changed nothing
        undetected += 1
    assert at == len(out)
    print("qpack corruption: %d of 60 single-bit flips in the strands decode without an error" % undetected)


@pytest.mark.parametrize("which", ["markov", "iid", "eight_bin"])
def test_packed_file_is_no_larger_than_bz2_and_xz(which):
    import numpy as np
    import harc_amd
    n, L = 20000, 100
    text = qc.markov(n, L, seed=1) if which == "markov" else qc.iid(n) if which == "iid" else qc.eight_bin(n, L)
    assert len(text) == n * (L + 1)
    packed = harc_amd.qpack_host(text, L)
    assert harc_amd.qunpack_host(packed) == text
    # the order-1 empirical entropy of the one block, with the block's contexts: the symbol in front, a context of its own for the first column
    a = np.frombuffer(text, dtype=np.uint8).reshape(n, L + 1)[:, :L].astype(np.int64)
    ctx = np.concatenate([np.full((n, 1), 255, dtype=np.int64), a[:, :-1]], axis=1)
    pair = np.bincount((ctx * 256 + a).ravel(), minlength=65536).reshape(256, 256).astype(np.float64)
    row = pair.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        bits = -np.nansum(np.where(pair > 0, pair * np.log2(pair / row), 0.0))
    entropy = bits / 8
    zb, zx = len(bz2.compress(text, 9)), len(lzma.compress(text, preset=6))
    print("qpack size %s: %d bytes of text -> %d; bz2 -9 %d (ratio %.4f), xz -6 %d (ratio %.4f), order-1 entropy %.0f bytes (packed / entropy %.4f)"
          % (which, len(text), len(packed), zb, len(packed) / zb, zx, len(packed) / zx, entropy, len(packed) / entropy))
    assert len(packed) <= zb and len(packed) <= zx
    assert len(packed) >= entropy


def test_bound_header_flag_and_the_empty_file():
    import harc_amd
    assert harc_amd.qpack_bound(0, 100) == 32
    assert harc_amd.qpack_bound(1, 100) == 32 + 5 + 100
    assert harc_amd.qpack_bound(41943, 100) == 32 + 5 + 4194300 and harc_amd.qpack_bound(41944, 100) == 32 + 10 + 4194400      # the default block of L = 100
    assert harc_amd.qpack_bound(16449, 255) == 32 + 2 * 5 + 16449 * 255                                                          # ... of L = 255: 16 448
    assert harc_amd.qpack_bound(901, 50, 300) == 32 + 4 * 5 + 45050
    text = qc.markov(901, 50, seed=3)
    f = harc_amd.qpack_host(text, 50, 300)
    assert f == _header(text, 50, 300) + harc_amd.qpack_host(text, 50, 300, header=False)
    assert f != harc_amd.qpack_host(text, 50) and harc_amd.qunpack_host(harc_amd.qpack_host(text, 50)) == text
    # block b of the file is the file of its lines alone
    assert f[32:] == b"".join(harc_amd.qpack_host(text[a * 51:(a + 300) * 51], 50, 300, header=False) for a in range(0, 901, 300))
    empty = harc_amd.qpack_host(b"", 37)
    assert empty == MAGIC + bytes(24) and harc_amd.qunpack_host(empty) == b""
    with pytest.raises(harc_amd.HarcAmdError) as e:                # a newline inside a line, none at the stride
        harc_amd.qpack_host(b"II\nIIII\n", 3)
    assert e.value.code == EINVAL
