"""BGZF input without a GPU: the member decoder of harc_amd/csrc/inflate_member.h built for the host with g++ and AddressSanitizer /
UBSan and fuzzed against zlib (the same source the inflate kernel compiles), run on crafted members that zlib's encoder never writes
(tests/foreign_deflate_cases.py), and the refusals that come before any device call."""
import os
import random
import shutil
import struct
import subprocess
import zlib
import gzip

import pytest

from tests import bgzf_util as bu
from tests import deflate_craft as dc
from tests import foreign_deflate_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include "inflate_member.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
// cases: [u32 n][n bytes] -> [i32 rc][u32 text bytes][text].  Every buffer is a heap block of exactly its size: a read or write past it is
// an AddressSanitizer report.
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint32_t crc[256];
    for (uint32_t i = 0; i < 256; i++) crc[i] = im_crc_entry(i);
    uint32_t n;
    while (fread(&n, 4, 1, f) == 1) {
        uint8_t *p = (uint8_t *)malloc(n ? n : 1);
        if (n && fread(p, 1, n, f) != n) return 3;
        uint32_t cap = 0, bs = 0, hdr = 0;
        if (im_bgzf_header(p, n, &bs, &hdr) && (uint64_t)bs + 1 <= n) cap = im_le32(p + bs + 1 - 4);
        if (cap > 65536) cap = 0;
        uint8_t *out = (uint8_t *)malloc(cap ? cap : 1);
        ImTables *t = (ImTables *)malloc(sizeof(ImTables));
        uint32_t mb = 0, tb = 0;
        const int32_t rc = im_member(p, n, out, cap, *t, crc, &mb, &tb);
        const uint32_t len = rc == 0 ? tb : 0;
        fwrite(&rc, 4, 1, o); fwrite(&len, 4, 1, o);
        if (len) fwrite(out, 1, len, o);
        free(t); free(out); free(p);
    }
    fclose(o); fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def decoder(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the host form of inflate_member.h")
    d = tmp_path_factory.mktemp("im")
    src = d / "drv.cpp"
    src.write_text(DRIVER)
    exe = d / "drv"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-Wall", "-Werror", "-I", os.path.join(ROOT, "harc_amd", "csrc"), str(src), "-o", str(exe)])

    def run(cases):
        cin, cout = d / "in.bin", d / "out.bin"
        with open(cin, "wb") as f:
            for c in cases:
                f.write(struct.pack("<I", len(c)) + c)
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


def _specials():
    """texts with matches at distance 1, of length 258 and as far back as zlib's encoder goes: within its window less 262 bytes (MAX_DIST), 32 506 at the most"""
    specials = [b"A" * 65536, b"AC" * 32768, bytes(range(256)) * 128 + b"x" * 32768, os.urandom(32768)[:100] + b"\0" * 200 + b"Q" * 258,
                (b"@" + os.urandom(16).hex().encode() + b"\n") * 1000]
    half = bytes(random.Random(11).getrandbits(8) for _ in range(32768))
    specials.append(b"ACGT" * 64 + half[:32000] + b"ACGT" * 64)                # a match 32 000+ back
    specials.append(half[:20000] + b"\n" + half[:20000])                      # distance 20 001
    specials.append(b"Z" + bytes(32767) + b"Z" + bytes(258))                   # a period of 32 768 that zlib codes at distance 1
    out = []
    for s in specials:
        for level in (1, 6, 9):
            for strat in ("default", "fixed", "rle"):
                try:
                    out.append((s, bu.member(s, level, strat, extra_before=b"XY\x03\x00abc" if level == 6 else b"")))
                except ValueError:
                    pass
    return out


def valid_corpus():
    """(text, member bytes): FASTQ-like and random text, levels 0-9, every zlib strategy, sizes 0 / 1 / 65 280 / 65 536, matches at distance 1, up to
    32 506 back (zlib's farthest) and of length 258, extra subfields in front of BC, and one member that zlib does not write: matches of length 258 at
    distance 32 768 (far_32768 of tests/foreign_deflate_cases.py)"""
    rng = random.Random(7)
    fq = bu.fastq_text(1200, 100, seed=3)
    out = []
    for level in range(10):
        for strat in bu.STRATEGIES:
            sizes = [0, 1, 17, 301, 4099, 65280, 65536] + [rng.randrange(2, 65536) for _ in range(14)]
            for size in sizes:
                for kind in ("fastq", "random"):
                    if kind == "fastq":
                        a = rng.randrange(0, len(fq) - size) if size < len(fq) else 0
                        text = fq[a:a + size]
                    else:
                        text = bytes(rng.getrandbits(8) for _ in range(min(size, 4099)))
                    try:
                        out.append((text, bu.member(text, level, strat)))
                    except ValueError:                            # incompressible 64 KiB does not fit one member (bgzip uses 65 280)
                        pass
    out += _specials()
    m, text = fc.bgzf_members()["far_32768"]
    out.append((text, m))
    out.append((b"", bu.EOF_MARKER))
    return out


def test_the_corpus_reaches_32768_only_in_its_crafted_member():
    far = [dc.max_distance(blocks) for _, m in _specials() for blocks in dc.gz_tokens(m)]
    assert max(far) <= 32506, max(far)
    (blocks,) = dc.gz_tokens(valid_corpus()[-2][1])
    assert (258, 32768) in [t for blk in blocks for t in blk["tokens"]]


def test_host_decoder_equals_zlib_on_valid_members(decoder):
    corpus = valid_corpus()
    assert len(corpus) >= 2000, len(corpus)
    res = decoder([m for _, m in corpus])
    bad = [i for i, ((text, _), (rc, got)) in enumerate(zip(corpus, res)) if rc != 0 or got != text]
    assert not bad, f"{len(bad)} members differ, first {bad[:5]}: rc {[res[i][0] for i in bad[:5]]}"


class BitWriter:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, val, bits):
        self.v |= (val & ((1 << bits) - 1)) << self.n
        self.n += bits

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def _crafted_bad_codes():
    """dynamic blocks whose code-length sets are over-subscribed or incomplete (rejected before any table lookup)"""
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    out = []
    # code-length code: 19 codes of length 1 (over-subscribed)
    w = BitWriter(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(15, 4)
    for _ in range(19):
        w.put(1, 3)
    out.append(w.bytes() + b"\0" * 8)
    # code-length code with a single code of length 2 (incomplete)
    w = BitWriter(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(15, 4)
    for k in range(19):
        w.put(2 if k == 3 else 0, 3)
    out.append(w.bytes() + b"\0" * 8)
    # complete code-length code (symbols 1 and 2, one bit each), then 258 literal / length and distance lengths of 1: over-subscribed
    w = BitWriter(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(14, 4)
    for k in range(18):
        w.put(1 if order[k] in (1, 2) else 0, 3)
    for _ in range(258):
        w.put(0, 1)                                               # symbol 1 (code 0): length 1
    out.append(w.bytes() + b"\0" * 8)
    # the same with lengths 2 for every symbol: 257 literal codes of 2 bits (over-subscribed as well)
    w = BitWriter(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(14, 4)
    for k in range(18):
        w.put(1 if order[k] in (1, 2) else 0, 3)
    for _ in range(258):
        w.put(1, 1)                                               # symbol 2 (code 1): length 2
    out.append(w.bytes() + b"\0" * 8)
    # no end-of-block code: literal 0 alone has a length (plus one distance code)
    w = BitWriter(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(14, 4)
    for k in range(18):
        w.put(1 if order[k] in (0, 1) else 0, 3)
    w.put(1, 1)                                                   # symbol 1 for literal 0 (code 1: symbols 0 and 1 have codes 0 and 1)
    for _ in range(256):
        w.put(0, 1)                                               # symbol 0: length 0
    w.put(1, 1)                                                   # the distance code: length 1
    out.append(w.bytes() + b"\0" * 8)
    return out


def _literal_only_member(text):
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    w = BitWriter(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(14, 4)
    for k in range(18):                                           # code-length code: symbols 0, 1, 2 with lengths 1, 2, 2 (codes 0, 10, 11)
        w.put({0: 1, 1: 2, 2: 2}.get(order[k], 0), 3)
    lens = [0] * 258
    lens[ord("A")] = 1
    lens[ord("C")] = lens[256] = 2                                # A = 0, C = 10, end-of-block = 11; the one distance length is 0
    cl = {0: (0, 1), 1: (0b10, 2), 2: (0b11, 2)}
    for v in lens:
        code, n = cl[v]
        for b in range(n - 1, -1, -1):                            # Huffman codes go first bit first
            w.put((code >> b) & 1, 1)
    sym = {ord("A"): (0, 1), ord("C"): (0b10, 2), 256: (0b11, 2)}
    for ch in list(text) + [256]:
        code, n = sym[ch]
        for b in range(n - 1, -1, -1):
            w.put((code >> b) & 1, 1)
    return bu.member(text, cdata=w.bytes())


def test_host_decoder_accepts_a_block_without_distance_codes(decoder):
    texts = [b"A", b"AC" * 300, b"CCCA" * 1000, b""]
    res = decoder([_literal_only_member(t) for t in texts])
    assert [r for r in res] == [(0, t) for t in texts]


def test_host_decoder_on_crafted_members_under_sanitizers(decoder):
    """streams that zlib does not write, each as the CDATA of one member: full tables with 15-bit codes and a run of code 16 that crosses from one tree into
    the other, runs of zeros that cross, a single distance code, no distance code, a block of end-of-block alone, empty blocks of every type, distance
    32 768; and the headers and symbols that zlib refuses, each with the code of its kind"""
    good = fc.bgzf_members()
    (blocks,) = dc.gz_tokens(good["full_tables"][0])
    assert all((b["hlit"], b["hdist"], b["maxbits"], b["cross"]) == (29, 29, (15, 15), 16) for b in blocks[:4]) and {b["cross_at"] for b in blocks[:4]} == {-1, 0}
    assert {b["cross"] for b in dc.gz_tokens(good["far_32768"][0])[0]} == {None, 17, 18}
    bad = fc.bgzf_refused_members()
    res = decoder([m for m, _ in good.values()] + list(bad.values()))
    assert res[:len(good)] == [(0, text) for _, text in good.values()], [(n, rc) for n, (rc, _) in zip(good, res) if rc]
    want = {"hlit": 4, "hdis": 4, "repe": 4, "run_": 4, "litl": 4, "fixe": 5, "stor": 3, "dist": 6}     # IM_E_CODES, IM_E_SYMBOL, IM_E_STORED, IM_E_DIST
    assert [rc for rc, _ in res[len(good):]] == [want[n[:4]] for n in bad], list(zip(bad, res[len(good):]))


def test_host_decoder_rejects_mutations_under_sanitizers(decoder):
    rng = random.Random(99)
    fq = bu.fastq_text(700, 100, seed=5)
    base = []
    for level, strat in [(1, "default"), (6, "default"), (9, "filtered"), (6, "huffman"), (6, "rle"), (6, "fixed"), (0, "default")]:
        a = rng.randrange(0, len(fq) - 30000)
        text = fq[a:a + rng.choice([3000, 12000, 30000])]
        base.append((text, bu.member(text, level, strat), bu.deflate_raw(text, level, strat)))
    cases, kinds = [], []
    for text, m, cd in base:
        hdr = 18
        for _ in range(250):                                      # one bit flipped inside CDATA
            b = bytearray(m)
            k = rng.randrange(hdr, len(m) - 8)
            b[k] ^= 1 << rng.randrange(8)
            cases.append(bytes(b)); kinds.append(("flip", text))
        for _ in range(20):                                       # CDATA cut short, BSIZE and trailer consistent with the cut
            cut = rng.randrange(0, len(cd))
            cases.append(bu.member(text, cdata=cd[:cut])); kinds.append(("trunc", None))
        for _ in range(10):                                       # the member itself cut short
            cases.append(m[:rng.randrange(0, len(m))]); kinds.append(("short", None))
        for d in (1, -1, 7, len(text) + 1, 70000):
            cases.append(bu.member(text, isize=len(text) + d)); kinds.append(("isize", None))
        for d in (1, -1, 3):
            cases.append(bu.member(text, crc=zlib.crc32(text) ^ d)); kinds.append(("crc", None))
        for d in (-1, -5, 1, 9):                                  # BSIZE one off: the trailer is read from the wrong place or past the end
            try:
                cases.append(bu.member(text, bsize_delta=d)); kinds.append(("bsize", None))
            except ValueError:
                pass
    for bad in _crafted_bad_codes():
        for isize in (0, 1, 100):
            cases.append(bu.member(b"x" * isize, cdata=bad)); kinds.append(("codes", None))
    assert len(cases) >= 2000, len(cases)
    res = decoder(cases)
    errs = 0
    for (kind, text), (rc, got) in zip(kinds, res):
        if kind == "flip":
            assert rc != 0 or got == text                         # a flip in the padding behind the last block changes nothing
            errs += rc != 0
        else:
            assert rc != 0, kind
            errs += 1
        if kind == "codes":
            assert rc == 4                                        # IM_E_CODES: refused before a single table lookup
    assert errs >= 0.95 * len(cases)


def test_compress_fastq_refuses_plain_gzip_without_a_device(tmp_path):
    """a single-stream .gz cannot be cut into pieces: refused with EINVAL before harc_amd_create (so also without a GPU)"""
    import harc_amd
    fq = tmp_path / "x.fastq.gz"
    fq.write_bytes(gzip.compress(bu.fastq_text(50)))
    os.makedirs(tmp_path / "output")
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.compress_fastq(str(fq), str(tmp_path), 100)
    assert e.value.code == -1 and "BGZF" in str(e.value), str(e.value)


def test_multi_gpu_refuses_bgzf_without_a_device(tmp_path):
    import harc_amd
    fq = tmp_path / "x.fastq.gz"
    fq.write_bytes(bu.bgzf(bu.fastq_text(50), member_text=4099))
    os.makedirs(tmp_path / "output")
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.compress_fastq_shard(str(fq), str(tmp_path), 100, 2, 0, "mailbox:" + str(tmp_path / "mb"), preserve_order=True)
    assert e.value.code == -1 and "BGZF" in str(e.value), str(e.value)
