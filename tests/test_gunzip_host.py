"""Plain gzip input without a GPU: the chunked inflate of harc_amd/csrc/inflate_stream.h built for the host with g++ and AddressSanitizer / UBSan into a
stand-alone driver and fuzzed against zlib (the same source the kernels compile), harc_amd_gunzip_host (the restatement that the device is held to) on every
case of tests/gunzip_cases.py, the paths it takes (starts found in parallel, repairs, dropped starts), the refusals, and ./harc with stand-in stage programs.
Both the driver and harc_amd_gunzip_host also run the streams of tests/foreign_deflate_cases.py, which zlib's encoder never writes, and the facts that give those
streams their names are stated here with the token reader of tests/deflate_craft.py."""
import gzip
import os
import random
import re
import shutil
import stat
import struct
import subprocess
import sys
import tarfile
import zlib

import pytest

from tests import bgzf_util as bu
from tests import deflate_craft as dc
from tests import foreign_deflate_cases as fc
from tests import gunzip_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include "inflate_stream.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
// cases: [u32 n][u32 chunk bytes][n bytes] -> [i32 rc][u32 text bytes][text].  The chunked algorithm in a row: the finder and a count pass for every chunk,
// the chain with its repairs, the write pass, the window step, the translation, CRC-32 and ISIZE.  Every buffer is a heap block of exactly its size: a read
// or write past it is an AddressSanitizer report.
struct Walk { uint64_t bit, end_bit, text; };
static uint32_t crc32_of(const uint8_t *p, size_t n, const uint32_t *tab)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t k = 0; k < n; k++) c = tab[(c ^ p[k]) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}
static int run(const uint8_t *p, uint64_t n, uint64_t cb, ImTables *t, const uint32_t *crctab, uint8_t **text_out, uint64_t *text_n)
{
    uint8_t *text = (uint8_t *)malloc(1); uint64_t tn = 0;
    *text_out = text; *text_n = 0;
    uint64_t pos = 0; int members = 0;
    while (pos < n) {
        uint64_t hdr = 0;
        int rc = gz_header(p + pos, n - pos, &hdr);
        if (rc) return members && rc == IM_E_GZHEADER ? IM_E_TRAILING : rc;
        const uint64_t base = pos; uint64_t e = (pos + hdr) * 8;
        const uint64_t nk = (n - base + cb - 1) / cb, k0 = ((e >> 3) - base) / cb;
        uint64_t *cand = (uint64_t *)malloc(sizeof(uint64_t) * nk); IsWalk *res = (IsWalk *)malloc(sizeof(IsWalk) * nk); int *rcs = (int *)malloc(sizeof(int) * nk);
        for (uint64_t k = k0 + 1; k < nk; k++) {
            const uint64_t hi = base + (k + 1) * cb < n ? base + (k + 1) * cb : n;
            cand[k] = is_find(p, n, (base + k * cb) * 8, hi * 8, *t);
            rcs[k] = cand[k] == IS_NONE ? -1 : is_count(p, n, cand[k], hi * 8, *t, &res[k]);
        }
        Walk *walks = (Walk *)malloc(sizeof(Walk) * (nk + 1)); uint64_t nw = 0, total = 0; int final = 0; rc = 0;
        while ((e >> 3) < n && nw <= nk) {
            const uint64_t k = ((e >> 3) - base) / cb, hi = base + (k + 1) * cb < n ? base + (k + 1) * cb : n;
            IsWalk w;
            if (k > k0 && cand[k] == e && rcs[k] == 0) w = res[k];
            else if ((rc = is_count(p, n, e, hi * 8, *t, &w))) break;
            if (w.end_bit == e) break;
            walks[nw].bit = e; walks[nw].end_bit = w.end_bit; walks[nw].text = w.text; nw++;
            total += w.text; e = w.end_bit;
            if (w.final) { final = 1; break; }
            if (w.more) break;
        }
        free(cand); free(res); free(rcs);
        if (!rc && !final) rc = IM_E_TRUNC;
        const uint64_t tb = (e + 7) >> 3;
        if (!rc && tb + 8 > n) rc = IM_E_TRUNC;
        if (rc) { free(walks); return rc; }
        // write pass, window step, translation
        uint8_t *win = (uint8_t *)calloc(IS_WIN, 1); uint32_t have = 0;
        text = (uint8_t *)realloc(text, tn + total ? tn + total : 1); *text_out = text;
        const uint64_t member_at = tn;
        for (uint64_t i = 0; i < nw && !rc; i++) {
            uint16_t *sym = (uint16_t *)malloc(walks[i].text ? 2 * walks[i].text : 1);
            IsWalk w;
            rc = is_walk(p, n, walks[i].bit, walks[i].end_bit, *t, sym, walks[i].text, &w);
            if (!rc && (w.end_bit != walks[i].end_bit || w.text != walks[i].text)) rc = IM_E_SHORT;
            for (uint64_t k = 0; k < walks[i].text && !rc; k++) rc = is_translate(sym[k], win, have, text + tn + k);
            if (!rc) {
                uint8_t *next = (uint8_t *)malloc(IS_WIN);
                for (uint32_t j = 0; j < IS_WIN; j++) next[j] = is_window_byte(win, sym, walks[i].text, j);
                free(win); win = next;
                have = is_window_have(have, walks[i].text); tn += walks[i].text;
            }
            free(sym);
        }
        free(win); free(walks);
        if (rc) return rc;
        *text_n = tn;
        if (crc32_of(text + member_at, tn - member_at, crctab) != im_le32(p + tb)) return IM_E_CRC;
        if ((uint32_t)(tn - member_at) != im_le32(p + tb + 4)) return IM_E_LENGTH;
        pos = tb + 8; members++;
    }
    return members ? IM_OK : IM_E_GZHEADER;
}
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint32_t crc[256];
    for (uint32_t i = 0; i < 256; i++) crc[i] = im_crc_entry(i);
    uint32_t n, cb;
    while (fread(&n, 4, 1, f) == 1 && fread(&cb, 4, 1, f) == 1) {
        uint8_t *p = (uint8_t *)malloc(n ? n : 1);
        if (n && fread(p, 1, n, f) != n) return 3;
        ImTables *t = (ImTables *)malloc(sizeof(ImTables));
        uint8_t *text = NULL; uint64_t tn = 0;
        const int32_t rc = run(p, n, cb, t, crc, &text, &tn);
        const uint32_t len = rc == 0 ? (uint32_t)tn : 0;
        fwrite(&rc, 4, 1, o); fwrite(&len, 4, 1, o);
        if (len) fwrite(text, 1, len, o);
        free(text); free(t); free(p);
    }
    fclose(o); fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def decoder(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the host form of inflate_stream.h")
    d = tmp_path_factory.mktemp("is")
    src = d / "drv.cpp"
    src.write_text(DRIVER)
    exe = d / "drv"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-Wall", "-Werror", "-I", os.path.join(ROOT, "harc_amd", "csrc"), str(src), "-o", str(exe)])

    def run(cases):
        """cases: (gzip bytes, chunk bytes) -> (rc, text)"""
        cin, cout = d / "in.bin", d / "out.bin"
        with open(cin, "wb") as f:
            for c, cb in cases:
                f.write(struct.pack("<II", len(c), cb) + c)
        r = subprocess.run([str(exe), str(cin), str(cout)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
        res, b, at = [], open(cout, "rb").read(), 0
        while at < len(b):
            rc, n = struct.unpack_from("<iI", b, at)
            res.append((rc, b[at + 8:at + 8 + n]))
            at += 8 + n
        assert len(res) == len(cases)
        return res
    return run


def _fuzz_texts(rng):
    fq = bu.fastq_text(900, 100, seed=5)
    half = bytes(rng.getrandbits(8) for _ in range(20000))
    return [fq, fq[:30000], half + b"\n" + half + fq[:5000] + half[:9000], b"A" * 70000 + b"AC" * 20000, b"", b"x", bytes(rng.getrandbits(8) for _ in range(3000))]


def test_driver_equals_zlib_under_sanitizers(decoder):
    """every strategy and level, chunk sizes from 64 bytes up, headers with every optional field, several members"""
    rng = random.Random(17)
    cases, want = [], []
    for text in _fuzz_texts(rng):
        for level, strat in [(1, "default"), (6, "default"), (9, "filtered"), (6, "huffman"), (6, "rle"), (6, "fixed"), (0, "default")]:
            blob = gc.gz_member(text, level, strat)
            for cb in (64, rng.randrange(65, 3000), rng.randrange(3000, 40000), 1 << 18):
                cases.append((blob, cb)); want.append(text)
    for name, (blob, text) in gc.valid_cases().items():
        if name[0] in "def":
            for cb in (64, 4099, 32768):
                cases.append((blob, cb)); want.append(text)
    res = decoder(cases)
    bad = [i for i, (w, (rc, got)) in enumerate(zip(want, res)) if rc != 0 or got != w]
    assert not bad, f"{len(bad)} of {len(cases)} differ, first {bad[:5]}: rc {[res[i][0] for i in bad[:5]]}"


def test_driver_refuses_bit_flips_under_sanitizers(decoder):
    """300 single-bit flips: any result is the text or an error code, never a sanitizer report; flips outside MTIME / XFL / OS are refused"""
    rng = random.Random(23)
    texts = _fuzz_texts(rng)[:4]
    cases, meta = [], []
    for _ in range(300):
        text = rng.choice(texts)
        level, strat = rng.choice([(1, "default"), (6, "default"), (9, "filtered"), (6, "huffman"), (6, "rle"), (6, "fixed"), (0, "default")])
        blob = bytearray(gc.gz_member(text, level, strat))
        k = rng.randrange(len(blob))
        blob[k] ^= 1 << rng.randrange(8)
        cases.append((bytes(blob), rng.choice([64, 500, 8192, 32768, 1 << 18]))); meta.append((text, 4 <= k < 10))
    for name, blob in gc.damaged_cases().items():
        cases.append((blob, 32768)); meta.append((None, False))
    res = decoder(cases)
    strict = refused = 0
    for (text, free), (rc, got) in zip(meta, res):
        assert rc != 0 or got == text
        if text is None:
            assert rc != 0
        if not free:
            strict += 1; refused += rc != 0
    assert refused >= 0.95 * strict, (refused, strict)


# ---------------------------------------------------------------------------------------------------------------- streams that zlib never writes
FOREIGN_CHUNKS = (64, 257, 1000, 4099, 32768, 1 << 18)
HOST_CHUNKS = (64, 1000, 32768, 0)


def _all_tokens(blocks):
    return [t for blk in blocks for t in blk["tokens"]]


def test_zlib_streams_stop_at_distance_32506():
    """what the crafted streams are for: zlib's encoder keeps a match within its window less 262 bytes (MAX_DIST), so no case of tests/gunzip_cases.py reaches
    indices 0 to 261 of the window in front of a walk"""
    far = {name: max(dc.max_distance(blocks) for blocks in dc.gz_tokens(blob)) for name, (blob, _) in gc.valid_cases().items()}
    assert max(far.values()) <= 32506, far


def test_foreign_families_hold_what_their_names_say():
    """facts about the streams of tests/foreign_deflate_cases.py, read back with the token reader"""
    got = {name: dc.gz_tokens(blob) for name, (blob, _) in fc.valid_cases().items()}
    for name, ms in got.items():                                    # the reader sees the text that zlib sees
        assert b"".join(dc.expand(_all_tokens(blocks)) for blocks in ms) == fc.valid_cases()[name][1], name
    for D in fc.FAR:
        (blocks,) = got[f"far_{D}"]
        lit, rest = [b for b in blocks if not any(isinstance(t, tuple) for t in b["tokens"])], blocks[-6:]
        assert len(lit) + 6 == len(blocks) and all(b["type"] == 2 and not b["final"] and 200 <= len(b["tokens"]) <= 900 for b in lit), D
        assert sum(len(b["tokens"]) for b in lit) == D + 3000
        assert {b["maxbits"][0] == 15 for b in lit} == {True, False} and {b["cross"] for b in lit} == {None, 17, 18}
        assert {b["ncodes"][1] for b in lit} >= {0, 2}              # no distance code at all, and codes that nothing uses
        assert [b["tokens"] for b in rest] == [[(L, D)] for L in (3, 258, 4, 257, 130)] + [[(258, D), (258, 1), (258, D), (3, D)]]
        assert all(b["ncodes"] == (2, 1) for b in rest[:5]) and rest[-1]["final"]
        assert dc.max_distance(blocks) == D
    (blocks,) = got["full_tables"]
    assert len(blocks) == 5 and all((b["hlit"], b["hdist"], b["maxbits"], b["ncodes"], b["cross"]) == (29, 29, (15, 15), (286, 30), 16) for b in blocks[:4])
    assert [b["cross_at"] for b in blocks[:4]] == [-1, 0, -1, 0]    # a run of code 16 over the boundary, and one that starts on it and repeats the other tree's length
    (blocks,) = got["one_dist_and_empties"]
    assert [b["type"] for b in blocks] == [2, 2, 2, 0, 1, 2]
    assert blocks[0]["ncodes"][1] == 1 and dc.max_distance(blocks[:1]) == 3
    assert blocks[1]["ncodes"][1] == 0 and len(blocks[1]["tokens"]) > 100
    assert blocks[2]["ncodes"] == (1, 0) and blocks[2]["maxbits"] == (1, 0)
    assert [blocks[k]["tokens"] for k in (2, 3, 4)] == [[], [], []]
    assert blocks[5]["tokens"] == [88] + [(258, 1)] * 300 and blocks[5]["ncodes"] == (3, 1)
    (blocks,) = got["pigz_like"]
    assert [b["type"] for b in blocks] == [2, 0, 0] * 5 + [1] and all(not b["tokens"] for b in blocks if b["type"] != 2) and blocks[-1]["final"]
    (blocks,) = got["empty_walks"]
    runs, k = [], 0
    while k < len(blocks):
        j = k
        while j < len(blocks) and blocks[j]["type"] == 0 and not blocks[j]["tokens"]:
            j += 1
        if j > k:
            runs.append((k, j)); k = j
        else:
            k += 1
    assert [j - k for k, j in runs] == [60, 60]
    for k, j in runs:                                               # longer than a chunk of 64 or 100 bytes, and the match behind them reaches over them
        assert blocks[j]["bit"] - blocks[k]["bit"] >= 300 * 8 - 7
        assert blocks[j]["tokens"][0][1] > 1
    assert blocks[runs[0][1]]["tokens"][0] == (100, 1500) and blocks[runs[1][1]]["tokens"][0] == (258, 1800)
    (blocks,) = got["stored_65535"]
    assert [(b["type"], len(b["tokens"])) for b in blocks] == [(0, 65535), (2, 10), (0, 65535), (1, 2), (0, 0)] and blocks[-1]["final"]
    assert blocks[1]["tokens"] == [(258, 32768)] * 10 and blocks[3]["tokens"] == [(258, 32768), (3, 32768)]
    assert len(fc.valid_cases()["stored_65535"][0]) > 1024 * 64    # more chunks of 64 bytes than the finder has waves
    (blocks,) = got["starts_behind_1024_chunks"]
    assert [b["type"] for b in blocks] == [0, 0] + [2] * 7 and [b["final"] for b in blocks] == [0] * 8 + [1]
    at = [(10 * 8 + b["bit"]) // 8 // 64 for b in blocks[2:]]       # the chunk of 64 bytes that holds each start
    assert at[0] >= 2048 and all(y > x for x, y in zip(at, at[1:])), at      # chunk 0 has the member's start: the finder's wave for chunk k is k - 1
    (blocks,) = got["fixed_only_far"]
    assert all(b["type"] == 1 for b in blocks) and dc.max_distance(blocks) == 32768
    first, second = got["two_members"]
    assert dc.max_distance(first) <= 32506 and dc.max_distance(second) == 32768


def test_driver_on_foreign_streams_under_sanitizers(decoder):
    """every family of tests/foreign_deflate_cases.py at six chunk sizes: the text that zlib gives, or for a stream that zlib refuses a code other than 0"""
    cases, want = [], []
    for name, (blob, text) in fc.valid_cases().items():
        for cb in FOREIGN_CHUNKS:
            cases.append((blob, cb)); want.append((name, cb, text))
    for name, (blob, _, _, _) in fc.refused_cases().items():
        for cb in FOREIGN_CHUNKS:
            cases.append((blob, cb)); want.append((name, cb, None))
    res = decoder(cases)
    bad = [(name, cb, rc) for (name, cb, text), (rc, got) in zip(want, res) if (rc != 0 or got != text) if text is not None]
    assert not bad, bad[:8]
    bad = [(name, cb) for (name, cb, text), (rc, got) in zip(want, res) if text is None and rc == 0]
    assert not bad, bad[:8]


def _stats_hold(st, blob, text, cb):
    ms = dc.gz_tokens(blob)
    assert st["members"] == len(ms) and st["text_bytes"] == len(text), st
    assert st["starts_dropped"] <= st["starts_found"] <= st["chunks"], st
    assert len(ms) <= st["chunks"] <= len(ms) * ((len(blob) + cb - 1) // cb), st     # a member's chunks are cut from its header to the end of the input
    assert st["repair_walks"] <= sum(len(blocks) for blocks in ms), st              # a repair takes the chain over a block at least


@pytest.mark.parametrize("name", sorted(fc.valid_cases()))
def test_gunzip_host_returns_the_text_of_foreign_streams(name):
    import harc_amd
    blob, text = fc.valid_cases()[name]
    for cb in HOST_CHUNKS:
        got, st = harc_amd.gunzip_host(blob, cb)
        assert got == text, (name, cb, st)
        _stats_hold(st, blob, text, cb or 256 << 10)


def test_the_chain_lands_on_starts_behind_1024_chunks():
    """what makes the finder's stride visible in the statistics that the device is held to: of the six non-final dynamic blocks that start in chunks 2048 and up,
    each alone in its chunk, at least five are found and used (a bit offset in front of one, in the same chunk, may parse as a header by accident)"""
    import harc_amd
    blob, text = fc.valid_cases()["starts_behind_1024_chunks"]
    got, st = harc_amd.gunzip_host(blob, 64)
    assert got == text and st["chunks"] > 2048 and st["starts_found"] - st["starts_dropped"] >= 5, st


@pytest.mark.parametrize("name", sorted(fc.refused_cases()))
def test_gunzip_host_refuses_what_zlib_refuses(name):
    """every refusal names a compressed byte inside the input; with the whole input in one chunk it is a byte of the first block of the member that is refused: a
    decode error is reported where it showed, a distance before the member's start at the first byte of the walk, and both lie in that block"""
    import harc_amd
    blob, lo, hi, _ = fc.refused_cases()[name]
    for cb in HOST_CHUNKS:
        with pytest.raises(harc_amd.HarcAmdError) as e:
            harc_amd.gunzip_host(blob, cb)
        m = re.search(r"compressed byte (\d+)", str(e.value))
        assert e.value.code == -1 and m and int(m.group(1)) <= len(blob), (cb, str(e.value))
        if cb == 0:
            assert lo <= int(m.group(1)) <= hi, (lo, hi, str(e.value))


@pytest.mark.parametrize("D", fc.FAR)
def test_gunzip_host_budget_turns_carry_the_window(D, monkeypatch):
    """HARC_AMD_GUNZIP_BUDGET cuts a member's text into turns, and the window goes from turn to turn in GzState::win.  A cut shows in the statistics: the chunks
    behind it are counted again.  At chunks of 1000 bytes and a budget of 41 000 the text of these streams (D + 4429 bytes, 37 197 at most) fits one turn.  35 000
    cuts the longer ones inside their D + 3000 literals: a walk there holds the literals of less than 1000 compressed bytes and of one more block, some 2000, so
    the first turn leaves a full window.  At chunks of 64 bytes a walk is one literal block, a budget of exactly the D + 3000 literals ends the first turn
    behind the last of them, and the second turn's first token is (3, D): with D = 32 768 it reads byte 0 of the carried window"""
    import harc_amd
    blob, text = fc.valid_cases()[f"far_{D}"]
    plain = {cb: harc_amd.gunzip_host(blob, cb)[1] for cb in (64, 1000)}
    for cb, budget in ((1000, 41000), (1000, 35000), (64, D + 3000)):
        monkeypatch.setenv("HARC_AMD_GUNZIP_BUDGET", str(budget))
        got, st = harc_amd.gunzip_host(blob, cb)
        assert got == text, (cb, budget)
        assert (st["chunks"] > plain[cb]["chunks"]) == (len(text) > budget), (cb, budget, st, plain[cb])
        assert (st["members"], st["text_bytes"]) == (1, len(text))


@pytest.mark.parametrize("name", sorted(gc.valid_cases()))
def test_gunzip_host_returns_the_text(name):
    import harc_amd
    blob, text = gc.valid_cases()[name]
    for cb in gc.CHUNKS:
        got, st = harc_amd.gunzip_host(blob, cb)
        assert got == text and st["text_bytes"] == len(text), (name, cb, st)
        assert st["members"] == (3 if name.startswith("d_") else 1)
        assert st["starts_dropped"] <= st["starts_found"] <= st["chunks"]


def test_crc_fold_agrees_with_zlib_at_span_boundaries():
    """the CRC-32 of a member is folded from 64-byte spans and 16 KiB tiles: lengths at and next to every boundary pass, and a CRC that is one bit off does not"""
    import harc_amd
    base = bu.fastq_text(400, 100, seed=8)
    for n in (0, 1, 63, 64, 65, 127, 128, 129, 16383, 16384, 16385, 16384 + 63, 16384 + 64, 16384 + 65, 32767, 32768, 32769, 49152 + 1):
        text = base[:n]
        got, _ = harc_amd.gunzip_host(gzip.compress(text, 6), 0)
        assert got == text, n
        with pytest.raises(harc_amd.HarcAmdError) as e:
            harc_amd.gunzip_host(gc.gz_member(text, 6, crc=zlib.crc32(text) ^ 0x80), 0)
        assert "CRC-32" in str(e.value), n


def test_the_parallel_path_produces_the_text():
    """(a) at level 6 in chunks of 32 KiB: the blocks are 19-20 KB of compressed bytes, so every chunk behind the first holds a start, the chain lands on every
    one of them and nothing is repaired"""
    import harc_amd
    blob, text = gc.valid_cases()["a_level6"]
    got, st = harc_amd.gunzip_host(blob, 32 << 10)
    assert got == text
    assert (st["chunks"], st["starts_found"], st["repair_walks"], st["starts_dropped"]) == (10, 9, 0, 0), st


def test_the_serial_paths_produce_the_text():
    import harc_amd
    blob, text = gc.valid_cases()["a_level6"]
    got, st = harc_amd.gunzip_host(blob, 8 << 10)                   # most chunks hold no start
    assert got == text and st["starts_found"] < st["chunks"] // 2, st
    blob, text = gc.valid_cases()["b_stored"]
    got, st = harc_amd.gunzip_host(blob, 32 << 10)                  # stored blocks are never found: every walk is a repair
    assert got == text and st["starts_found"] == 0 and st["repair_walks"] > 0, st
    blob, text = gc.valid_cases()["f_deflate_inside_stored"]
    got, st = harc_amd.gunzip_host(blob, 32 << 10)                  # starts that parse inside stored data are all false
    assert got == text and st["starts_dropped"] > 0 and st["starts_dropped"] == st["starts_found"], st


@pytest.mark.parametrize("name", sorted(gc.damaged_cases()))
def test_damage_is_refused_naming_a_compressed_byte(name):
    import harc_amd
    blob = gc.damaged_cases()[name]
    for cb in gc.CHUNKS:
        with pytest.raises(harc_amd.HarcAmdError) as e:
            harc_amd.gunzip_host(blob, cb)
        assert e.value.code == -1 and re.search(r"compressed byte \d+", str(e.value)), str(e.value)


def test_no_gzip_at_all_is_refused():
    import harc_amd
    for blob in (b"", b"@r1\nACGT\n+\nIIII\n", b"\x1f\x8b\x07\x00" + bytes(20), b"\x1f\x8b\x08\x20" + bytes(20)):
        with pytest.raises(harc_amd.HarcAmdError) as e:
            harc_amd.gunzip_host(blob, 0)
        assert e.value.code == -1 and "compressed byte 0" in str(e.value), str(e.value)


def test_compress_fastq_still_refuses_plain_gzip(tmp_path):
    """the text is handed to the ingest as a file (./harc); the file-level call keeps refusing a single-stream .gz before any device call"""
    import harc_amd
    fq = tmp_path / "x.fastq.gz"
    fq.write_bytes(gzip.compress(bu.fastq_text(50)))
    os.makedirs(tmp_path / "output")
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.compress_fastq(str(fq), str(tmp_path), 100)
    assert e.value.code == -1 and "BGZF" in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------------------------- ./harc with stand-in stage programs
STUB = r"""#!/bin/bash
# stand-in for harc_amd_stage: records the commands; gunzip is Python's gzip, or fails after leaving half a file (STUB_GUNZIP=fail)
set -e
cmd=$1; base=$2; out=$base/output
streams()
{
    for s in read_seq read_pos read_noise read_noisepos read_rev; do printf 'AAAA' > $out/$s.txt.0; done
    printf 'AC' > $out/read_seq.txt.0.tail; printf '1' > $out/read_rev.txt.0.tail
    printf 'ACGT\n' > $out/input_N.dna; printf 'G' > $out/read_singleton.txt; printf 'T' > $out/read_singleton.txt.tail
    printf '100\n' > $out/read_meta.txt
    for s in read_order.bin read_order_N.bin read_order_N_pe.bin numreads.bin; do printf 'xxxx' > $out/$s; done
}
case $cmd in
gunzip)
    echo "gunzip $2 $3 $4" >> "$STUB_LOG"
    if [[ "$STUB_GUNZIP" == "fail" ]]; then printf '@half' > "$4"; echo "stub: gunzip refuses" >&2; exit 1; fi
    "$STUB_PY" -c 'import gzip, sys; open(sys.argv[2], "wb").write(gzip.open(sys.argv[1]).read())' "$2" "$4"
    echo "[gunzip] 1 members, 1 chunks, 0 starts found, 0 dropped, 0 repaired, $(wc -c < "$4") bytes of text"
    exit 0;;
compressfq)
    echo "$cmd $3 $4" >> "$STUB_LOG"
    cp "$4" "$STUB_LOG.$cmd.input"
    streams
    exit 0;;
pack_order) printf 'tail' > $out/read_order.bin.tail;;
*) echo "stub: unknown command $cmd"; exit 1;;
esac
"""


def _setup(tmp_path, **more):
    stub = tmp_path / "stage_stub.sh"
    stub.write_text(STUB)
    stub.chmod(stub.stat().st_mode | stat.S_IXUSR)
    text = bu.fastq_text(300, 100, seed=1)
    env = dict(os.environ, HARC_AMD_STAGE_BIN=str(stub), HARC_AMD_STAGE3="none", STUB_LOG=str(tmp_path / "stub.log"), STUB_PY=sys.executable, **more)
    if "HARC_AMD_GUNZIP" not in more:
        env.pop("HARC_AMD_GUNZIP", None)
    gz = tmp_path / "y.fq.gz"
    gz.write_bytes(gzip.compress(text))
    return text, gz, env


def _run(args, env):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _names(arc):
    with tarfile.open(arc) as tf:
        return sorted(os.path.basename(n) for n in tf.getnames() if os.path.basename(n) not in ("", "."))


def _log(tmp_path):
    return [l.split() for l in (tmp_path / "stub.log").read_text().splitlines()]


def test_harc_inflates_plain_gzip_with_the_stage_program(tmp_path):
    text, gz, env = _setup(tmp_path, HARC_AMD_GUNZIP="1")
    r = _run(["-c", str(gz)], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "[gunzip] 1 members" in r.stdout and "on the host" not in r.stdout
    log = _log(tmp_path)
    assert log[0][:3] == ["gunzip", str(gz), "0"] and log[0][3].endswith("output/.input.fastq")
    assert log[1][0] == "compressfq" and log[1][1] == "100" and log[1][2].endswith("output/.input.fastq") and len(log) == 2
    assert (tmp_path / "stub.log.compressfq.input").read_bytes() == text
    names = _names(tmp_path / "y.fq.harc")
    assert ".input.fastq" not in names and ".gunzip.err" not in names and "read_meta.txt" in names
    assert not (tmp_path / "output").exists()


def test_harc_falls_back_to_the_host_when_the_stage_program_fails(tmp_path):
    text, gz, env = _setup(tmp_path, HARC_AMD_GUNZIP="1")
    assert _run(["-c", str(gz)], env).returncode == 0
    want = _names(tmp_path / "y.fq.harc")
    os.remove(tmp_path / "y.fq.harc"); os.remove(tmp_path / "stub.log")
    r = _run(["-c", str(gz)], dict(env, STUB_GUNZIP="fail"))
    assert r.returncode == 0, r.stdout[-2000:]
    assert "expanding it on the host" in r.stdout and "bgzip" in r.stdout and "[gunzip]" not in r.stdout
    log = _log(tmp_path)
    assert [l[0] for l in log] == ["gunzip", "compressfq"]
    assert (tmp_path / "stub.log.compressfq.input").read_bytes() == text       # not the half file the failed call left
    assert _names(tmp_path / "y.fq.harc") == want


@pytest.mark.parametrize("setting", ["0", None])
def test_harc_skips_the_gpu_attempt_unless_asked_for_it(setting, tmp_path):
    """the GPU inflate is slower than the host's gzip so far (NOTES.md): it runs with HARC_AMD_GUNZIP=1 only"""
    text, gz, env = _setup(tmp_path, **({"HARC_AMD_GUNZIP": setting} if setting else {}))
    r = _run(["-c", str(gz)], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "expanding it on the host" in r.stdout
    assert [l[0] for l in _log(tmp_path)] == ["compressfq"]
    assert (tmp_path / "stub.log.compressfq.input").read_bytes() == text


def test_harc_keeps_bgzf_with_g_on_the_host(tmp_path):
    text, gz, env = _setup(tmp_path, HARC_AMD_GUNZIP="1")
    bz = tmp_path / "z.fastq.gz"
    bz.write_bytes(bu.bgzf(text, 4099))
    r = _run(["-c", str(bz), "-g", "2", "-p"], env)
    assert "expanding it on the host" in r.stdout
    assert not (tmp_path / "stub.log").exists() or all(l[0] != "gunzip" for l in _log(tmp_path))
