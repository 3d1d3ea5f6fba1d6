"""The recovery record without a GPU: the arithmetic of harc_amd/csrc/gf_block.h (the source the kernels compile) built for the host with g++, AddressSanitizer and
UBSan as a stand-alone program and held to the tables of tests/recovery_cases.py; what the library's host twin writes against the record the plain Python reference
makes from the README's format text, byte for byte; every damage pattern repaired or refused as the reference repairs or refuses it."""
import os
import random
import shutil
import struct
import subprocess

import pytest

from harc_amd import api
from tests import recovery_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EIO = -1, -3
PAIRS = [(1, 1), (2, 1), (5, 3), (100, 20), (128, 7), (128, 128)]

DRIVER = r"""
#include "gf_block.h"
#include <stdio.h>
#include <stdlib.h>
// tables:  -> 65536 products a * b (byte a * 256 + b), 256 inverses (0 for 0)
// words:   [u32 n][n words] -> for c = 0 .. 255: the n packed products
// coef:    problems [u32 k][u32 e][e lost][e rec] -> [u32 ok][e * k coefficients]
// head:    records [u32 bytes][the record] -> [u32 found][u32 which]; every record is a heap block of exactly its size
int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    FILE *f = fopen(argv[2], "rb"), *o = fopen(argv[3], "wb");
    if (!f || !o) return 2;
    uint32_t n;
    if (!strcmp(argv[1], "tables")) {
        for (uint32_t a = 0; a < 256; a++) for (uint32_t b = 0; b < 256; b++) fputc((int)gf_mul(a, b), o);
        for (uint32_t a = 0; a < 256; a++) fputc((int)gf_inv(a), o);
    } else if (!strcmp(argv[1], "words")) {
        if (fread(&n, 4, 1, f) != 1) return 3;
        uint32_t *w = (uint32_t *)malloc(4 * (size_t)n);
        if (fread(w, 4, n, f) != n) return 3;
        for (uint32_t c = 0; c < 256; c++) for (uint32_t k = 0; k < n; k++) { const uint32_t r = gf_mul_word(w[k], c); fwrite(&r, 4, 1, o); }
        free(w);
    } else if (!strcmp(argv[1], "coef")) {
        uint32_t k, e;
        while (fread(&k, 4, 1, f) == 1 && fread(&e, 4, 1, f) == 1) {
            uint32_t *lost = (uint32_t *)malloc(4 * (size_t)e), *rec = (uint32_t *)malloc(4 * (size_t)e);
            if (fread(lost, 4, e, f) != e || fread(rec, 4, e, f) != e) return 3;
            uint8_t *coef = (uint8_t *)malloc((size_t)e * k);
            const uint32_t ok = gf_repair_coef(k, lost, rec, (int)e, coef);
            fwrite(&ok, 4, 1, o); fwrite(coef, 1, (size_t)e * k, o);
            free(coef); free(rec); free(lost);
        }
    } else if (!strcmp(argv[1], "head")) {
        while (fread(&n, 4, 1, f) == 1) {
            uint8_t *p = (uint8_t *)malloc(n ? n : 1);
            if (n && fread(p, 1, n, f) != n) return 3;
            GfHead H; int which = 0; std::string why;
            const uint32_t found = gf_head_find([&](uint64_t off, uint64_t len, uint8_t *dst) { if (off + len > n) return false; memcpy(dst, p + off, (size_t)len); return true; },
                                                (uint64_t)n, &H, &which, &why);
            const uint32_t w = (uint32_t)which;
            fwrite(&found, 4, 1, o); fwrite(&w, 4, 1, o);
            free(p);
        }
    } else return 2;
    fclose(o); fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the host form of gf_block.h")
    d = tmp_path_factory.mktemp("gf")
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
    return rc.cases()


@pytest.fixture(scope="module")
def records(cases):
    """the reference's record of every case, made once"""
    return {c["name"]: rc.make_record(c["files"], c["PCT"], c["B"], c["S"], c["K"]) for c in cases}


# ------------------------------------------------------------------------------------------------ the arithmetic
def test_all_products_and_inverses_equal_the_python_tables(driver):
    out = driver("tables", b"")
    assert len(out) == 65536 + 256
    assert out[:65536] == bytes(rc.mul(a, b) for a in range(256) for b in range(256))
    assert out[65536] == 0 and out[65537:] == bytes(rc.inv(a) for a in range(1, 256))
    assert all(rc.mul(a, rc.inv(a)) == 1 for a in range(1, 256))


def test_the_packed_word_product_equals_the_bytewise_one_for_all_256_coefficients(driver):
    rnd = random.Random(11)
    words = [0, 0xFFFFFFFF, 0x80808080, 0x7F7F7F7F, 0x01020408, 0x8040201D] + [rnd.getrandbits(32) for _ in range(250)]
    out = driver("words", struct.pack("<I%dI" % len(words), len(words), *words))
    got = struct.unpack("<%dI" % (256 * len(words)), out)
    for c in range(256):
        for k, w in enumerate(words):
            want = int.from_bytes(bytes(rc.mul(c, b) for b in w.to_bytes(4, "little")), "little")
            assert got[c * len(words) + k] == want, (c, hex(w))


def _ref_coef(k, lost, recs):
    Ainv = rc.invert([[rc.cauchy(i, j) for j in lost] for i in recs])
    keep = [j for j in range(k) if j not in lost]
    return [[_xor(rc.mul(Ainv[q][r], rc.cauchy(i, j)) for r, i in enumerate(recs)) for j in keep] + Ainv[q] for q in range(len(lost))]


def _xor(vals):
    v = 0
    for x in vals:
        v ^= x
    return v


def test_the_matrix_inverse_holds_on_seeded_erasure_patterns_for_the_six_pairs(driver):
    rnd = random.Random(5)
    problems = []
    for k, m in PAIRS:
        for e in sorted({1, min(k, m), max(1, min(k, m) // 2)}):
            for _ in range(3 if k < 100 else 1):
                problems.append((k, sorted(rnd.sample(range(k), e)), sorted(rnd.sample(range(m), e))))
    blob = b"".join(struct.pack("<II%dI%dI" % (len(l), len(r)), k, len(l), *l, *r) for k, l, r in problems)
    out, at = driver("coef", blob), 0
    for k, lost, recs in problems:
        e = len(lost)
        assert struct.unpack_from("<I", out, at)[0] == 1
        got = [list(out[at + 4 + q * k:at + 4 + (q + 1) * k]) for q in range(e)]
        at += 4 + e * k
        assert got == _ref_coef(k, lost, recs), (k, lost, recs)
        # and the coefficients do rebuild the lost members
        members = [bytes(rnd.getrandbits(8) for _ in range(4)) for _ in range(k)]
        rblocks = rc.combine(members, [[rc.cauchy(i, j) for j in range(k)] for i in recs])
        assert rc.combine([members[j] for j in range(k) if j not in lost] + rblocks, got) == [members[j] for j in lost]
    assert at == len(out)


# ------------------------------------------------------------------------------------------------ the record
def _lay_out(d, case, rec=None):
    """the files of a case (and a record) in the directory d -> (paths, the record's path)"""
    d.mkdir(exist_ok=True)
    paths = []
    for name, data in case["files"]:
        (d / name).write_bytes(data)
        paths.append(str(d / name))
    if rec is not None:
        (d / "x.hr").write_bytes(rec)
    return paths, str(d / "x.hr")


def _twin_make(d, case):
    paths, out = _lay_out(d, case)
    st = api.recovery_make_host(paths, case["PCT"], out=out, block_bytes=case["B"], span_blocks=case["S"], group_blocks=case["K"])
    return st, open(out, "rb").read()


def test_the_host_twin_writes_the_references_record_byte_for_byte(tmp_path, cases, records):
    for c in cases:
        st, got = _twin_make(tmp_path / c["name"], c)
        assert got == records[c["name"]], c["name"]
        H, which = rc.read_head(got)
        assert which == 1 and st["record_bytes"] == len(got) and st["files"] == len(c["files"]) and st["bytes"] == sum(len(x) for _, x in c["files"])
        assert st["blocks"] == sum(f["nb"] for f in H["files"])
        assert api.recovery_repair_host(str(tmp_path / c["name"] / "x.hr"), write=False) == (0, ["[recovery] %s ok" % n for n, _ in c["files"]])


def test_the_geometry_from_the_environment_is_recorded(tmp_path, monkeypatch, cases, records):
    c = next(x for x in cases if x["name"] == "spans3")
    monkeypatch.setenv("HARC_AMD_RECOVERY_BLOCK", str(c["B"]))
    monkeypatch.setenv("HARC_AMD_RECOVERY_SPAN", str(c["S"]))
    monkeypatch.setenv("HARC_AMD_RECOVERY_GROUP", str(c["K"]))
    paths, out = _lay_out(tmp_path / "env", c)
    api.recovery_make_host(paths, c["PCT"], out=out)
    assert open(out, "rb").read() == records["spans3"]
    os.remove(out)
    for name, val in (("HARC_AMD_RECOVERY_BLOCK", "24"), ("HARC_AMD_RECOVERY_GROUP", "129")):
        monkeypatch.setenv(name, val)
        with pytest.raises(api.HarcAmdError) as e:
            api.recovery_make_host(paths, c["PCT"], out=out)
        assert e.value.code == EINVAL and not os.path.exists(out)
        monkeypatch.setenv(name, str(c["B"] if "BLOCK" in name else c["K"]))


# ------------------------------------------------------------------------------------------------ repair
def _group_blocks(case, fi, sp, g):
    """the block numbers of group g of span sp of file fi of a case, and its (k, m)"""
    data = case["files"][fi][1]
    nb = -(-len(data) // case["B"])
    t0, s = rc.spans_of(nb, case["S"])[sp]
    G, groups = rc.groups_of_span(s, case["K"], case["PCT"])
    k, m = groups[g]
    return [t0 + j * G + g for j in range(k)], k, m, G


def _damage(data, B, blocks):
    x = bytearray(data)
    for t in blocks:
        x[t * B] ^= 0x40
    return bytes(x)


def _both(tmp, case, rec, files, write=True):
    """the reference and the host twin on the same damaged files -> the twin's (status, lines), after asserting that both agree on status, lines and bytes"""
    tmp.mkdir(exist_ok=True)
    for name, _ in case["files"]:
        p = tmp / name
        if files.get(name) is None:
            if p.exists():
                p.unlink()
        else:
            p.write_bytes(files[name])
    (tmp / "x.hr").write_bytes(rec)
    want = rc.repair(rec, "x.hr", files, write)
    got = api.recovery_repair_host(str(tmp / "x.hr"), write=write)
    assert got == want[:2], (got, want[:2])
    for name, _ in case["files"]:
        p = tmp / name
        assert (p.read_bytes() if p.exists() else None) == want[2].get(name), name
    assert (tmp / "x.hr").read_bytes() == rec                      # the record is never written
    return got


def test_a_single_flipped_bit_is_repaired(tmp_path, cases, records):
    for c in cases:
        fi = max(range(len(c["files"])), key=lambda i: len(c["files"][i][1]))
        name, data = c["files"][fi]
        files = dict(c["files"])
        x = bytearray(data)
        x[len(x) // 2] ^= 1
        files[name] = bytes(x)
        st, lines = _both(tmp_path / c["name"], c, records[c["name"]], files, write=False)
        assert st == 1 and "[recovery] %s damaged: 1 of %d blocks, recoverable" % (name, -(-len(data) // c["B"])) in lines
        st, lines = _both(tmp_path / c["name"], c, records[c["name"]], files)
        assert st == 0 and "[recovery] %s repaired: 1 of %d blocks" % (name, -(-len(data) // c["B"])) in lines
        assert (tmp_path / c["name"] / name).read_bytes() == data


def test_exactly_m_lost_members_are_recovered_and_m_plus_1_refused_in_every_case(tmp_path, cases, records):
    for c in cases:
        for fi, (name, data) in enumerate(c["files"]):
            if not data:
                continue
            blocks, k, m, G = _group_blocks(c, fi, 0, 0)
            files = dict(c["files"])
            files[name] = _damage(data, c["B"], blocks[-min(k, m):])                     # (the file's last block among them where the group holds it)
            st, lines = _both(tmp_path / c["name"], c, records[c["name"]], files)
            assert st == 0 and (tmp_path / c["name"] / name).read_bytes() == data, (c["name"], name, lines)
            if k > m:
                files[name] = _damage(data, c["B"], blocks[:m + 1])
                st, lines = _both(tmp_path / c["name"], c, records[c["name"]], files)
                assert st == 1 and "[recovery] %s NOT recoverable: span 0 group 0 has lost %d of %d blocks and holds %d recovery blocks" % (name, m + 1, k, m) in lines
                assert (tmp_path / c["name"] / name).read_bytes() == files[name]         # the file's bytes unchanged


def test_a_burst_of_G_m_blocks_is_recovered_and_one_more_from_a_group_boundary_refused(tmp_path, cases, records):
    c = next(x for x in cases if x["name"] == "b48")              # G = 2, k = 3, m = 2
    name, data = c["files"][0]
    _, k, m, G = _group_blocks(c, 0, 0, 0)
    assert (G, k, m) == (2, 3, 2)
    files = {name: _damage(data, c["B"], range(1, 1 + G * m))}
    st, lines = _both(tmp_path / "burst", c, records["b48"], files)
    assert st == 0 and lines == ["[recovery] %s repaired: %d of 6 blocks" % (name, G * m)]
    files = {name: _damage(data, c["B"], range(0, G * m + 1))}
    st, lines = _both(tmp_path / "burst", c, records["b48"], files)
    assert st == 1 and lines == ["[recovery] %s NOT recoverable: span 0 group 0 has lost 3 of 3 blocks and holds 2 recovery blocks" % name]


def test_a_truncated_file_a_missing_file_and_a_longer_file(tmp_path, cases, records):
    c = next(x for x in cases if x["name"] == "m128")             # PCT = 100
    name, data = c["files"][0]
    for cut in (len(data) - 1, len(data) - 16 * 5 - 3, 16, 0):
        st, lines = _both(tmp_path / "cut", c, records["m128"], {name: data[:cut]})
        assert st == 0 and (tmp_path / "cut" / name).read_bytes() == data, cut
    st, lines = _both(tmp_path / "gone", c, records["m128"], {name: None}, write=False)
    assert st == 1 and lines == ["[recovery] %s damaged: 128 of 128 blocks, recoverable" % name] and not (tmp_path / "gone" / name).exists()
    st, lines = _both(tmp_path / "gone", c, records["m128"], {name: None})
    assert st == 0 and lines == ["[recovery] %s repaired: 128 of 128 blocks" % name] and (tmp_path / "gone" / name).read_bytes() == data
    # three files, the empty one missing: it is created
    c3 = next(x for x in cases if x["name"] == "three")
    files = dict(c3["files"])
    files["f1.bin"] = None
    st, lines = _both(tmp_path / "three", c3, records["three"], files)
    assert st == 0 and (tmp_path / "three" / "f1.bin").read_bytes() == b""
    # a longer file: refused naming both lengths, nothing written
    (tmp_path / "long").mkdir()
    _lay_out(tmp_path / "long", c, records["m128"])
    (tmp_path / "long" / name).write_bytes(data[:5] + b"!" + data[5:])
    with pytest.raises(rc.Refused):
        rc.repair(records["m128"], "x.hr", {name: data[:5] + b"!" + data[5:]})
    with pytest.raises(api.HarcAmdError) as e:
        api.recovery_repair_host(str(tmp_path / "long" / "x.hr"))
    assert e.value.code == EINVAL and "holds 2049 bytes" in str(e.value) and "records 2048" in str(e.value)
    assert (tmp_path / "long" / name).read_bytes() == data[:5] + b"!" + data[5:]


def _flip_recovery_block(rec, r, B):
    H, _ = rc.read_head(rec)
    x = bytearray(rec)
    x[H["hb"] + r * B + 3] ^= 0x10
    return bytes(x)


def test_a_damaged_recovery_block_alone_and_together_with_m_minus_1_lost_members(tmp_path, cases, records):
    c = next(x for x in cases if x["name"] == "b48")
    name, data = c["files"][0]
    rec = _flip_recovery_block(records["b48"], 0, c["B"])
    st, lines = _both(tmp_path / "r", c, rec, dict(c["files"]))
    assert st == 0 and lines == ["[recovery] x.hr: 1 of 4 recovery blocks damaged", "[recovery] %s ok" % name]
    st, lines = _both(tmp_path / "r", c, rec, dict(c["files"]), write=False)
    assert st == 1                                                 # -n: status 0 only when nothing at all is damaged
    blocks, k, m, G = _group_blocks(c, 0, 0, 0)
    files = {name: _damage(data, c["B"], blocks[:m - 1])}
    st, lines = _both(tmp_path / "r", c, rec, files)               # recovered from the other recovery block
    assert st == 0 and lines[-1] == "[recovery] %s repaired: 1 of 6 blocks" % name and (tmp_path / "r" / name).read_bytes() == data
    files = {name: _damage(data, c["B"], blocks[:m])}
    st, lines = _both(tmp_path / "r", c, rec, files)
    assert st == 1 and lines[-1] == "[recovery] %s NOT recoverable: span 0 group 0 has lost 2 of 3 blocks and holds 1 recovery blocks" % name


def test_head_copy_one_damaged_and_both_damaged(tmp_path, cases, records, driver):
    c = next(x for x in cases if x["name"] == "three")
    rec = records["three"]
    H, _ = rc.read_head(rec)
    one = bytearray(rec)
    one[60] ^= 1
    name, data = c["files"][0]
    files = dict(c["files"])
    files[name] = _damage(data, c["B"], [2])
    st, lines = _both(tmp_path / "h", c, bytes(one), files)
    assert st == 0 and lines[0] == "[recovery] x.hr: the first copy of the head is damaged, the second holds" and (tmp_path / "h" / name).read_bytes() == data
    both = bytearray(one)
    both[len(rec) - 20] ^= 1
    (tmp_path / "h" / "x.hr").write_bytes(bytes(both))
    with pytest.raises(rc.Refused):
        rc.read_head(bytes(both))
    with pytest.raises(api.HarcAmdError) as e:
        api.recovery_repair_host(str(tmp_path / "h" / "x.hr"))
    assert e.value.code == EINVAL and "the first copy" in str(e.value) and "the second copy" in str(e.value)
    # a record cut short, and one that is missing
    (tmp_path / "h" / "x.hr").write_bytes(rec[:-9])
    with pytest.raises(api.HarcAmdError) as e:
        api.recovery_repair_host(str(tmp_path / "h" / "x.hr"))
    assert e.value.code == EINVAL
    os.remove(tmp_path / "h" / "x.hr")
    with pytest.raises(api.HarcAmdError) as e:
        api.recovery_repair_host(str(tmp_path / "h" / "x.hr"))
    assert e.value.code == EIO and "was not compressed with -P" in str(e.value)
    # under the sanitizers: the good record and the three damaged ones
    blobs = [rec, bytes(one), bytes(both), rec[:-9]]
    out = driver("head", b"".join(struct.pack("<I", len(b)) + b for b in blobs))
    assert struct.unpack("<8I", out) == (1, 1, 1, 2, 0, 0, 0, 0)


def _forged(rec, edit):
    """both head copies of rec edited by edit(bytearray head) and their digests made to hold again"""
    H, _ = rc.read_head(rec)
    hb = H["hb"]
    h = bytearray(rec[:hb])
    edit(h)
    h[40:48] = bytes(8)
    h[40:48] = struct.pack("<Q", rc.digest(bytes(h)))
    return bytes(h) + rec[hb:len(rec) - 8 - hb] + bytes(h) + rec[-8:]


def test_a_head_whose_counts_exceed_the_file_and_a_name_with_a_slash_are_refused(tmp_path, cases, records, driver):
    c = next(x for x in cases if x["name"] == "kK")
    rec = records["kK"]
    name = c["files"][0][0].encode()
    at = 48 + 2 + len(name)                                        # n, D, nb, recovery_blocks of the one file

    def huge(h):
        h[at:at + 8] = struct.pack("<Q", 1 << 50)
        h[at + 16:at + 32] = struct.pack("<QQ", 1 << 46, 1 << 44)

    def files_count(h):
        h[24:28] = struct.pack("<I", 0xFFFFFFFF)

    def slash(h):
        h[50:51] = b"/"

    forged = [_forged(rec, huge), _forged(rec, files_count), _forged(rec, slash)]
    for k, bad in enumerate(forged):
        _lay_out(tmp_path / ("f%d" % k), c, bad)
        with pytest.raises(rc.Refused):
            rc.read_head(bad)
        with pytest.raises(api.HarcAmdError) as e:
            api.recovery_repair_host(str(tmp_path / ("f%d" % k) / "x.hr"))
        assert e.value.code == EINVAL, str(e.value)
        assert (tmp_path / ("f%d" % k) / c["files"][0][0]).read_bytes() == c["files"][0][1]
    # without a large allocation: the same records through the parser under the sanitizers, each a heap block of exactly its size
    out = driver("head", b"".join(struct.pack("<I", len(b)) + b for b in forged + [rec]))
    assert struct.unpack("<8I", out) == (0, 0, 0, 0, 0, 0, 1, 1)
    # a record made over a name that is none
    with pytest.raises(api.HarcAmdError) as e:
        api.recovery_make_host([str(tmp_path) + "/.."], 5, out=str(tmp_path / "y.hr"))
    assert e.value.code == EINVAL and not (tmp_path / "y.hr").exists()
