"""Lossy quality values without a GPU: the spec strings and the table rule of harc_amd_qmap_parse, the serial mapper behind harc_amd_qmap_host against the Python
restatement of tests/qmap_cases.py (bytes and statistics), the promises of the run smoothing, the bodies of both kernels (harc_amd/csrc/qm_block.h, the source
that qmap.hip compiles) run with their lanes as loops in a stand-alone program built by g++ with AddressSanitizer and UBSan, and what the mapping is for: the
size of the packed quality file."""
import os
import shutil
import struct
import subprocess

import pytest

from tests import qmap_cases as mc
from tests import quality_cases as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
CASES = mc.cases()
ILL8_TABLE = (bytes(range(33)) + b"!!" + b"'" * 8 + b"0" * 10 + b"7" * 5 + b"<" * 5 + b"B" * 5 + b"F" * 5 + b"I" * 54 + bytes(range(127, 256)))


def test_every_valid_spec_parses_to_its_map():
    import harc_amd
    m = harc_amd.qmap_parse("ill8")
    assert (m.kind, bytes(m.table)) == (1, ILL8_TABLE) and len(ILL8_TABLE) == 256
    assert mc.table("ill8") == ILL8_TABLE                          # the twin's table is the literal one too
    for spec in ("bin:20:40:6", "bin:1:0:0", "bin:93:93:93", "bin:93:93:0", "cap:0", "cap:30", "cap:93"):
        m = harc_amd.qmap_parse(spec)
        assert (m.kind, bytes(m.table)) == (1, mc.table(spec)), spec
    for r in (1, 2, 4, 46):
        m = harc_amd.qmap_parse("pblock:%d" % r)
        assert (m.kind, m.radius) == (2, r)


@pytest.mark.parametrize("spec,named", [
    ("ill9", "ill9"), ("", "name"), ("ILL8", "ILL8"), ("ill8:1", "ill8:1"), ("ill8 ", "ill8 "),
    ("bin", "T"), ("bin:20", "H"), ("bin:20:40", "L"), ("bin:20:40:6:1", "behind L"), ("bin:0:40:6", "T = 0"), ("bin:94:40:6", "T = 94"),
    ("bin:20:94:6", "H = 94"), ("bin:20:6:40", "L = 40"), ("bin:20:40:-1", "L"), ("bin:2x:40:6", "T"),
    ("cap", "M"), ("cap:", "M"), ("cap:94", "M = 94"), ("cap:30x", "trailing"), ("cap:30 ", "trailing"), ("cap:3.5", "trailing"), ("cap: 30", "M"),
    ("pblock:0", "R = 0"), ("pblock:47", "R = 47"), ("pblock:2:2", "behind R"), ("pblock:+2", "R"), ("pblock:99999", "R"),
])
def test_malformed_specs_are_refused_by_name(spec, named):
    import harc_amd
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.qmap_parse(spec)
    assert e.value.code == EINVAL and ("'%s'" % spec) in str(e.value) and named in str(e.value), str(e.value)


def test_invalid_maps_are_refused_with_the_first_offending_byte():
    import harc_amd
    text = b"IIII\nHHHH\n"

    def refused(m, *words):
        with pytest.raises(harc_amd.HarcAmdError) as e:
            harc_amd.qmap_host(text, 4, m)
        assert e.value.code == EINVAL and all(w in str(e.value) for w in words), str(e.value)
    for v, to in ((10, 11), (32, 33), (127, 126), (255, 0), (0, 1)):          # a byte outside 33..126 that the table would change
        m = harc_amd.qmap_parse("ill8")
        m.table[v] = to
        if v != 255:
            m.table[255] = 7                                       # (a later one as well: the first is named)
        refused(m, "byte value %d " % v)
    for v, to in ((33, 32), (126, 127), (70, 10), (40, 255)):      # a value mapped out of 33..126
        m = harc_amd.qmap_parse("cap:30")
        m.table[v] = to
        if v != 126:
            m.table[126] = 5
        refused(m, "byte value %d " % v, "%d" % to)
    for kind in (0, 3, -1):
        m = harc_amd.qmap_parse("ill8")
        m.kind = kind
        refused(m, "kind %d" % kind)
    for r in (0, 47, -2):
        m = harc_amd.qmap_parse("pblock:3")
        m.radius = r
        refused(m, "radius %d" % r)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_mapper_is_the_python_twin_in_bytes_and_statistics(name):
    import harc_amd
    text, L = CASES[name]
    for spec in mc.SCHEMES:
        want, wstats = mc.mapped(text, L, spec)
        got, stats = harc_amd.qmap_host(text, L, spec)
        assert got == want, spec
        assert stats == wstats, spec
        assert harc_amd.qmap_host(text, L, spec, stats=False) == (want, None), spec


def test_run_smoothing_keeps_its_promises():
    import harc_amd
    for name in sorted(CASES):
        text, L = CASES[name]
        for r in (1, 2, 4, 46):
            got, stats = harc_amd.qmap_host(text, L, "pblock:%d" % r)
            assert len(got) == len(text) and stats["max_abs"] <= r
            for a, b in zip(text, got):
                if 33 <= a <= 126:
                    assert abs(a - b) <= r and 33 <= b <= 126
                else:
                    assert a == b                                  # newlines and bytes outside 33..126
    # what the cases are there for
    text, L = CASES["alternating_extremes"]
    assert harc_amd.qmap_host(text, L, "pblock:46")[0] == text     # 126 - 33 = 93 > 92: every byte is its own block
    text, L = CASES["one_block_lines"]
    assert set(harc_amd.qmap_host(text, L, "pblock:1")[0]) == {71, 10}
    # not idempotent: at R = 1 the line 60 62 63 is cut into 60 62 | 63 and becomes 61 61 63, which is one block and becomes 62 62 62
    once = harc_amd.qmap_host(bytes([60, 62, 63]) + b"\n", 3, "pblock:1")[0]
    assert once == bytes([61, 61, 63]) + b"\n" and harc_amd.qmap_host(once, 3, "pblock:1")[0] == bytes([62, 62, 62]) + b"\n"


def test_the_stride_check_is_the_packers(tmp_path):
    import harc_amd
    text, L = CASES["L100_300"]
    for at, byte, counts in ((150 * 101 + 40, 10, "0 positions on the 101-byte stride hold no newline and 1 newlines"),
                             (150 * 101 + 100, ord("I"), "1 positions on the 101-byte stride hold no newline and 0 newlines")):
        b = bytearray(text)
        b[at] = byte
        for spec in ("ill8", "pblock:2"):
            with pytest.raises(harc_amd.HarcAmdError) as e:
                harc_amd.qmap_host(bytes(b), L, spec)
            with pytest.raises(harc_amd.HarcAmdError) as ep:
                harc_amd.qpack_host(bytes(b), L)
            assert e.value.code == EINVAL and counts in str(e.value) and str(e.value) == str(ep.value), str(e.value)
    with pytest.raises(harc_amd.HarcAmdError):
        harc_amd.qmap_host(b"II\n", 0, "ill8")
    with pytest.raises(harc_amd.HarcAmdError):
        harc_amd.qmap_host(b"I" * 256 + b"\n", 256, "ill8")
    assert harc_amd.build_has("qmap")


# ------------------------------------------------------------------------------------------------ the kernels' bodies, lanes as loops, under the sanitizers
DRIVER = r"""
#include "qm_block.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
// cases [u32 n][u32 L][i32 kind][i32 radius][256 bytes table][n (L + 1) bytes] -> [u32 status][the serial mapper's n (L + 1) bytes].  The text of a run is the
// tail of a heap block that is exactly its 16-byte-aligned hull: a load that leaves the hull is an AddressSanitizer report.  The output has 0xEE bytes either side,
// inside its own hull.  status: 1 the lanes' bytes are not the serial mapper's, 2 their statistics are not, 4 a byte outside the output was written, 8 the counts
// of the stride check are not, 16 the input of an out-of-place run was changed
struct Placed { uint8_t *block, *p; size_t size; };
static Placed place(const uint8_t *src, size_t N, unsigned off)
{
    Placed P;
    P.size = (off + N + 15) & ~(size_t)15;
    if (!P.size) P.size = 16;
    if (posix_memalign((void **)&P.block, 16, P.size)) exit(3);
    memset(P.block, 0xEE, P.size);
    P.p = P.block + off;
    if (src) memcpy(P.p, src, N);
    return P;
}
static int guards_ok(const Placed &P, size_t N) { for (uint8_t *q = P.block; q < P.block + P.size; q++) if ((q < P.p || q >= P.p + N) && *q != 0xEE) return 0; return 1; }
static int same_acc(const QmAcc &a, const QmAcc &b) { return !memcmp(&a, &b, sizeof a); }

static void run_lanes(const uint8_t *in, uint8_t *out, uint64_t n, uint32_t L, const harc_amd_qmap &M, QmAcc *acc, uint64_t *err, uint64_t G)
{
    qm_acc_zero(acc); err[0] = err[1] = 0;
    const uint64_t N = n * (L + 1ull);
    if (M.kind == QM_KIND_TABLE) {
        uint64_t e[2] = { 0, 0 };
        uint8_t *table = (uint8_t *)malloc(256);                   // the kernel's copy in LDS
        memcpy(table, M.table, 256);
        for (uint64_t g = 0; g < G; g++) { QmAcc a; qm_acc_zero(&a); qm_table_item<true>(in, out, N, L, table, g, G, &a, e); qm_acc_merge(acc, &a); }
        free(table);
        err[0] = n - e[0]; err[1] = e[1] - e[0];
        return;
    }
    const uint32_t LL = L + 1, pitch = 4 * qm_pitch(L);
    uint8_t *rows = (uint8_t *)malloc((size_t)QM_TILE * pitch);
    for (uint64_t line0 = 0; line0 < n; line0 += QM_TILE) {
        const uint32_t m = n - line0 < QM_TILE ? (uint32_t)(n - line0) : QM_TILE, T = m * LL;
        memset(rows, 0xDD, (size_t)QM_TILE * pitch);
        for (uint32_t t = 0; t < QM_TILE; t++) qm_tile_load(in + line0 * LL, T, LL, pitch, rows, t, QM_TILE);
        for (uint32_t t = 0; t < QM_TILE; t++) { QmAcc a; qm_acc_zero(&a); qm_tile_walk<true>(rows, m, L, pitch, (uint32_t)M.radius, t, &a, err); qm_acc_merge(acc, &a); }
        for (uint32_t t = 0; t < QM_TILE; t++) qm_tile_store(out + line0 * LL, T, LL, pitch, rows, t, QM_TILE);
    }
    free(rows);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint32_t h[4];
    while (fread(h, 4, 4, f) == 4) {
        harc_amd_qmap M; memset(&M, 0, sizeof M);
        const uint64_t n = h[0]; const uint32_t L = h[1];
        M.kind = (int32_t)h[2]; M.radius = (int32_t)h[3];
        if (fread(M.table, 1, 256, f) != 256) return 3;
        const size_t N = (size_t)(n * (L + 1ull));
        uint8_t *text = (uint8_t *)malloc(N ? N : 1), *want = (uint8_t *)malloc(N ? N : 1);
        if (N && fread(text, 1, N, f) != N) return 3;
        QmAcc wacc; qm_acc_zero(&wacc);
        uint64_t werr[2] = { 0, 0 };
        qm_map_text<true>(text, n, L, &M, want, &wacc, werr);
        uint32_t st = 0;
        {   // the serial mapper in place, and without statistics
            uint8_t *again = (uint8_t *)malloc(N ? N : 1);
            memcpy(again, text, N);
            QmAcc a; qm_acc_zero(&a); uint64_t e[2] = { 0, 0 };
            qm_map_text<false>(again, n, L, &M, again, &a, e);
            if (memcmp(again, want, N)) st |= 1;
            free(again);
        }
        static const unsigned in_offs[4] = { 0, 1, 3, 15 }, out_offs[3] = { 0, 5, 8 };
        for (unsigned a = 0; a < 4; a++) {
            for (unsigned b = 0; b < 4; b++) {                     // b == 3: in place
                Placed I = place(text, N, in_offs[a]), O = b < 3 ? place(nullptr, N, 16 + out_offs[b]) : I;
                QmAcc acc; uint64_t err[2];
                run_lanes(I.p, O.p, n, L, M, &acc, err, a % 2 ? 48 : 272);
                if (memcmp(O.p, want, N)) st |= 1;
                if (!same_acc(acc, wacc)) st |= 2;
                if (!guards_ok(O, N)) st |= 4;
                if (err[0] != werr[0] || err[1] != werr[1]) st |= 8;
                if (b < 3 && (memcmp(I.p, text, N) || !guards_ok(I, N))) st |= 16;
                if (b < 3) free(O.block);
                free(I.block);
            }
        }
        fwrite(&st, 4, 1, o);
        fwrite(want, 1, N, o);
        free(want); free(text);
    }
    fclose(o); fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the host form of qm_block.h")
    d = tmp_path_factory.mktemp("qm")
    src = d / "drv.cpp"
    src.write_text(DRIVER)
    exe = d / "drv"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-Wall", "-Werror", "-I", os.path.join(ROOT, "harc_amd", "csrc"), str(src), "-o", str(exe)])

    def run(blob):
        cin, cout = d / "in.bin", d / "out.bin"
        cin.write_bytes(blob)
        r = subprocess.run([str(exe), str(cin), str(cout)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]                  # the sanitizers are silent
        return cout.read_bytes()
    return run


def test_kernel_bodies_with_lanes_as_loops_are_the_serial_mapper_under_the_sanitizers(driver):
    """every case and scheme, input offsets 0, 1, 3, 15 and output offsets 0, 5, 8 from a 16-byte boundary, in place and out of place, guard bytes either side"""
    import harc_amd
    jobs = []
    for name in sorted(CASES):
        text, L = CASES[name]
        for spec in mc.SCHEMES:
            m = harc_amd.qmap_parse(spec)
            jobs.append((name, spec, struct.pack("<IIii", len(text) // (L + 1), L, m.kind, m.radius) + bytes(m.table) + text))
    out, at = driver(b"".join(j[2] for j in jobs)), 0
    for name, spec, _ in jobs:
        text, L = CASES[name]
        st, = struct.unpack_from("<I", out, at)
        assert st == 0, (name, spec, st)
        assert out[at + 4:at + 4 + len(text)] == mc.mapped(text, L, spec)[0], (name, spec)
        at += 4 + len(text)
    assert at == len(out)
    # a text that fails the stride check: the lanes count what the serial mapper counts (status bit 8)
    text, L = CASES["L100_300"]
    b = bytearray(text)
    b[150 * 101 + 40], b[7 * 101 + 100], b[8 * 101 + 100] = 10, ord("I"), ord("J")
    blob = b""
    for spec in ("cap:30", "pblock:2"):
        m = harc_amd.qmap_parse(spec)
        blob += struct.pack("<IIii", 300, L, m.kind, m.radius) + bytes(m.table) + bytes(b)
    out = driver(blob)
    assert struct.unpack_from("<I", out, 0)[0] == 0 and struct.unpack_from("<I", out, 4 + len(b))[0] == 0


# ------------------------------------------------------------------------------------------------ what it is for
def test_the_packed_quality_file_shrinks_by_the_factors_of_the_entropy():
    """20 000 lines of 100: the packed size of the mapped text against that of the text.  The order-1 entropies put the ratios at 0.37 (markov, ill8), 0.41
    (markov, pblock:2) and 0.51 (iid, ill8); the packer stays within 2 % of the entropy"""
    import harc_amd
    n, L = 20000, 100
    for gen_name, text, bounds in (("markov", qc.markov(n, L), {"ill8": 0.6, "pblock:2": 0.6}), ("iid", qc.iid(n), {"ill8": 0.7})):
        base = len(harc_amd.qpack_host(text, L))
        for spec, bound in bounds.items():
            mapped, _ = harc_amd.qmap_host(text, L, spec, stats=False)
            size = len(harc_amd.qpack_host(mapped, L))
            print("%s %s: %d -> %d bytes, ratio %.3f" % (gen_name, spec, base, size, size / base))
            assert size <= bound * base, (gen_name, spec, size, base)
