"""The packed id file without a GPU: the block coder of harc_amd/csrc/id_block.h (the source the kernels compile) built for the host with g++, AddressSanitizer
and UBSan as a stand-alone program; what the library's host twin writes read back by a decoder in plain Python written from the README's format text; the
stored / coded mode of every block; damaged files refused; the size against bz2 and xz; the bound and the empty file."""
import bz2
import lzma
import os
import shutil
import struct
import subprocess

import pytest

from tests import id_cases as ic
from tests.readme_decoders import id_decode as readme_decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
MAGIC = b"HARCI1\0\0"

DRIVER = r"""
#include "id_block.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
// enc: cases [u32 text bytes][u32 rb][text] -> [u32 status][u32 bytes][the blocks, no file header].  Every buffer is a heap block of exactly its size: a read or
// write past it is an AddressSanitizer report.  status: 1 a second run into a block of the exact size differs, 2 id_block_decode does not return the text
// dec: files [u32 bytes][the file] -> [u32 code][u32 block][u32 text bytes][text]; code 0, an ID_E_* of the first bad block, 100 a prefix that leaves the file or
// the text, 101 the header, 200 the strands decoded one by one answer otherwise
static uint32_t one_block(const uint8_t *lines, uint32_t tb, uint32_t m, FILE *o, uint32_t *total)
{
    uint32_t st = 0;
    uint8_t *text = (uint8_t *)malloc(tb);                        // the block's lines alone
    memcpy(text, lines, tb);
    IdWork *W = (IdWork *)malloc(sizeof(IdWork));
    uint16_t *events = (uint16_t *)malloc(2 * id_block_events(tb, m));
    uint8_t *slabs = (uint8_t *)malloc(id_block_slabs(tb, m));
    uint8_t *big = (uint8_t *)malloc(9 + (size_t)tb);
    int stored = 0;
    const uint32_t size = id_block_encode(text, tb, m, *W, events, slabs, big, 9 + (size_t)tb, &stored);
    if (!size) return 4;
    uint8_t *exact = (uint8_t *)malloc(size);
    if (id_block_encode(text, tb, m, *W, events, slabs, exact, size, &stored) != size || memcmp(big, exact, size)) st |= 1;
    if (id_block_encode(text, tb, m, *W, events, slabs, exact, size - 1, &stored) != 0) st |= 1;
    uint8_t *payload = (uint8_t *)malloc(size - 4);
    memcpy(payload, exact + 4, size - 4);
    uint8_t *back = (uint8_t *)malloc(tb);
    if (qv_le32(exact) != size - 4 || qv_le32(payload + 1) != tb || id_block_decode(payload, size - 4, m, *W, back) != ID_OK || memcmp(back, text, tb)) st |= 2;
    fwrite(exact, 1, size, o); *total += size;
    free(back); free(payload); free(exact); free(big); free(slabs); free(events); free(W); free(text);
    return st;
}
// a coded block that id_block_decode has taken as far as its strands with the answer `code` (W holds its table): strand after strand on its own, from a heap block of
// exactly its coded bytes into one of exactly its text bytes -- a strand that wrote into its neighbour's text is an AddressSanitizer report here
static uint32_t strands_alone(const uint8_t *pl, uint32_t pbytes, uint32_t m, IdWork &W, const uint8_t *text, uint32_t code)
{
    uint32_t mode = 0, tbytes = 0, hdr1 = 0, bm[4], bad = ID_E_NONE, differs = 0, tat = 0;
    if (id_check_head(pl, pbytes, &mode, &tbytes, bm, &hdr1)) return 200;
    const uint8_t *src = pl + hdr1;
    for (uint32_t s = 0; s < ID_STRANDS; s++) {
        uint32_t st, sl;
        if (id_check_strand(pl, m, s, &st, &sl)) return 200;
        uint8_t *in = (uint8_t *)malloc(sl ? sl : 1), *out = (uint8_t *)malloc(st ? st : 1);
        memcpy(in, src, sl);
        const uint32_t e = id_code(id_strand_decode(in, sl, W.fc, out, st, id_strand_lines(m, s)));
        bad = id_min(bad, e);
        if (e == ID_E_NONE && memcmp(out, text + tat, st)) differs = 1;
        free(out); free(in);
        src += sl; tat += st;
    }
    if (differs || (bad == ID_E_NONE ? code != 0 : code != bad)) return 200;
    return code;
}
static void one_file(const uint8_t *f, uint32_t nbytes, FILE *o)
{
    uint32_t code = 0, tb = 0, block = 0;
    uint8_t *text = NULL;
    if (nbytes < 32 || !id_magic_ok(f) || qv_le32(f + 12)) code = 101;
    else {
        const uint32_t rb = qv_le32(f + 8); const uint64_t n = qv_le64(f + 16), tbytes = qv_le64(f + 24);
        if (n == 0) code = nbytes == 32 && !rb && !tbytes ? 0 : 101;
        else if (rb < 1 || n > 1000000 || tbytes > 100000000 || tbytes < n) code = 101;
        else {
            tb = (uint32_t)tbytes;
            text = (uint8_t *)malloc(tb);
            memset(text, 0, tb);
            IdWork *W = (IdWork *)malloc(sizeof(IdWork));
            uint64_t at = 32, tat = 0;
            for (uint64_t a = 0; a < n && !code; a += rb, block++) {
                const uint32_t m = n - a < rb ? (uint32_t)(n - a) : rb;
                if (nbytes - at < 9) { code = 100; break; }
                const uint32_t pb = qv_le32(f + at), t = qv_le32(f + at + 5);
                if (pb < 5 || nbytes - at - 4 < pb || t > tbytes - tat) { code = 100; break; }
                uint8_t *payload = (uint8_t *)malloc(pb), *lines = (uint8_t *)malloc(t ? t : 1);
                memcpy(payload, f + at + 4, pb);
                memset(lines, 0, t);
                code = (uint32_t)id_block_decode(payload, pb, m, *W, lines);
                if (payload[0] && (code == 0 || code >= ID_E_TRUNC)) code = strands_alone(payload, pb, m, *W, lines, code);
                memcpy(text + tat, lines, t);
                free(lines); free(payload);
                if (code) break;
                at += 4 + (uint64_t)pb; tat += t;
            }
            if (!code && (at != nbytes || tat != tbytes)) { code = 100; block--; }
            free(W);
        }
    }
    fwrite(&code, 4, 1, o); fwrite(&block, 4, 1, o); fwrite(&tb, 4, 1, o);
    if (tb) fwrite(text, 1, tb, o);
    free(text);
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
            uint32_t rb;
            if (fread(&rb, 4, 1, f) != 1) return 3;
            uint8_t *p = (uint8_t *)malloc(n ? n : 1);
            if (n && fread(p, 1, n, f) != n) return 3;
            if (!rb) rb = ID_DEFAULT_RB;
            uint32_t st = 0, total = 0;
            const long head = ftell(o);
            fwrite(&st, 4, 1, o); fwrite(&total, 4, 1, o);
            uint32_t a = 0;
            while (a < n) {
                uint32_t e = a, m = 0;
                while (e < n && m < rb) { while (p[e] != '\n') e++; e++; m++; }
                st |= one_block(p + a, e - a, m, o, &total);
                a = e;
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
        pytest.fail("g++ is needed to build the host form of id_block.h")
    d = tmp_path_factory.mktemp("idb")
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
    c = ic.small_cases()
    c.update({k: (v, 0) for k, v in ic.real_sets().items()})
    return c


def _header(text, rb):
    n = text.count(b"\n")
    return MAGIC + (struct.pack("<IIQQ", rb or 1 << 18, 0, n, len(text)) if n else bytes(24))


def test_every_case_round_trips_in_the_sanitizer_build(driver, cases):
    import harc_amd
    names = sorted(cases)
    out = driver("enc", b"".join(struct.pack("<II", len(cases[k][0]), cases[k][1]) + cases[k][0] for k in names))
    at = 0
    for k in names:
        st, n = struct.unpack_from("<II", out, at)
        blocks, at = out[at + 8:at + 8 + n], at + 8 + n
        assert st == 0, (k, st)
        text, rb = cases[k]
        assert _header(text, rb) + blocks == harc_amd.idpack_host(text, rb), k      # the library's host twin is this code
    assert at == len(out)


def test_a_decoder_written_from_the_readme_reads_every_case(cases):
    import harc_amd
    for k, (text, rb) in sorted(cases.items()):
        f = harc_amd.idpack_host(text, rb)
        got, modes = readme_decode(f)
        assert got == text, k
        assert harc_amd.idunpack_host(f) == text, k
        assert len(f) <= harc_amd.idpack_bound(len(text), text.count(b"\n"), rb), k
        assert modes == ic.MODES.get(k, [1]), (k, modes)            # what each case is there for; the three sets of 20 000 ids are one coded block


def test_corruption_is_refused(driver):
    import harc_amd
    text = ic.corruption_text()
    packed = harc_amd.idpack_host(text)
    bad = ic.corrupted(packed)
    names = sorted(bad)
    out = driver("dec", b"".join(struct.pack("<I", len(bad[k])) + bad[k] for k in names))          # the sanitizer build reports nothing on any of them
    at, undetected = 0, 0
    for k in names:
        code, block, tb = struct.unpack_from("<III", out, at)
        got, at = out[at + 12:at + 12 + tb], at + 12 + tb
        try:
            back = harc_amd.idunpack_host(bad[k])
        except harc_amd.HarcAmdError as e:
            assert e.code == EINVAL and code != 0, (k, code, str(e))
            if k != "wrong_magic":
                assert "block 0" in str(e) and block == 0, (k, str(e))
            if not k.startswith(("wrong", "trunc", "trailing", "payload", "header", "block_text")):
                assert "block 0 at byte 32 is damaged" in str(e), (k, str(e))
            continue
        assert k.startswith("flip") and code == 0 and back == text and got == text, k          # a flip that decodes without an error changed nothing
        undetected += 1
    assert at == len(out)
    assert undetected == 0, "%d of 60 single-bit flips in the strands decode without an error" % undetected


@pytest.mark.parametrize("which", ["illumina_in_order", "srr", "illumina_shuffled"])
def test_packed_size_against_bz2_and_the_text(which):
    import harc_amd
    text = ic.real_sets()[which]
    packed = harc_amd.idpack_host(text)
    assert harc_amd.idunpack_host(packed) == text
    zb, zx = len(bz2.compress(text, 9)), len(lzma.compress(text, preset=9))
    print("idpack size %s: %d bytes of text -> %d; bz2 -9 %d (ratio %.4f), xz -9 %d (ratio %.4f)" % (which, len(text), len(packed), zb, len(packed) / zb, zx, len(packed) / zx))
    if which == "illumina_shuffled":
        assert len(packed) < len(text)
    else:
        assert len(packed) < zb


def test_bound_header_flag_and_the_empty_file():
    import harc_amd
    assert harc_amd.idpack_bound(0, 0) == 32
    assert harc_amd.idpack_bound(71, 1) == 32 + 9 + 71
    assert harc_amd.idpack_bound(1000, (1 << 18) + 1) == 32 + 2 * 9 + 1000
    assert harc_amd.idpack_bound(45050, 901, 300) == 32 + 4 * 9 + 45050
    text, rb = ic.small_cases()["cut_901_RB300"]
    f = harc_amd.idpack_host(text, rb)
    assert f == _header(text, rb) + harc_amd.idpack_host(text, rb, header=False)
    assert f != harc_amd.idpack_host(text) and harc_amd.idunpack_host(harc_amd.idpack_host(text)) == text
    # block b of the file is the file of its lines alone
    lines = text.splitlines(keepends=True)
    assert f[32:] == b"".join(harc_amd.idpack_host(b"".join(lines[a:a + 300]), 300, header=False) for a in range(0, 901, 300))
    empty = harc_amd.idpack_host(b"")
    assert empty == MAGIC + bytes(24) and harc_amd.idunpack_host(empty) == b""
    with pytest.raises(harc_amd.HarcAmdError) as e:                # a last line without its newline
        harc_amd.idpack_host(b"@a 1\n@a 2")
    assert e.value.code == EINVAL and "newline" in str(e.value)
