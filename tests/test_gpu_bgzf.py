"""BGZF input inflated on the GPU: harc_amd_bgzf_inflate_device against zlib, compress_fastq on a BGZF file against the same call on the
plain file (every output file byte for byte, in every ingest mode), set_fastq_bgzf_device against set_fastq_device, and corrupt input
refused with EINVAL naming the member (the host build of the same decoder is fuzzed under sanitizers in tests/test_bgzf_host.py)."""
import os
import random
import zlib

import pytest

from tests import bgzf_util as bu
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu
ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda") if b else torch.empty(16, dtype=torch.uint8, device="cuda")


def _inflate(h, blob):
    import torch
    d = _dev(blob)
    n = h.bgzf_inflate_device(d.data_ptr(), len(blob))
    out = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    assert h.bgzf_inflate_device(d.data_ptr(), len(blob), out.data_ptr(), n) == n
    torch.cuda.synchronize()
    return out[:n].cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        yield h


def test_inflate_equals_zlib(ctx):
    rng = random.Random(5)
    fq = bu.fastq_text(7000, 100, seed=9)
    files = []
    for level, strat, size in [(0, "default", 65280), (1, "default", 65280), (6, "filtered", 4099), (9, "default", 301), (6, "huffman", 65280),
                               (6, "rle", 20000), (6, "fixed", 65280), (3, "default", 1)]:
        text = fq[:min(len(fq), size * 5000)] if size > 1 else fq[:3000]
        files.append((text, bu.bgzf(text, size, level, strat)))
    rnd = bytes(rng.getrandbits(8) for _ in range(300000))
    files.append((rnd, bu.bgzf(rnd, 65280, 6)))
    runs = b"A" * 70000 + b"AC" * 40000 + rnd[:40000] + rnd[:40000]
    files.append((runs, bu.bgzf(runs, 65536, 9, extra_before=b"XY\x02\x00zz")))
    files.append((fq[:5000] + fq[5000:9000], bu.bgzf(fq[:5000], 999) + bu.bgzf(fq[5000:9000], 777)))       # two BGZF files concatenated
    files.append((b"", bu.EOF_MARKER))
    files.append((b"", b""))
    for text, blob in files:
        assert _inflate(ctx, blob) == text
    assert len(bu.members(files[3][1])) >= 5000


def _compress(path, base, L, K, E, p=False, q=False):
    import harc_amd
    os.makedirs(os.path.join(base, "output"), exist_ok=True)
    harc_amd.compress_fastq(str(path), base, L, num_thr=E, num_chains=K, num_steps=16, preserve_order=p, preserve_quality=q)
    return ol.read_dir(base)


def _same_as_plain(tmp_path, text, L, member_text, K=1, E=1, p=False, q=False, tag="x"):
    plain, gz = tmp_path / f"{tag}.fastq", tmp_path / f"{tag}.fastq.gz"
    plain.write_bytes(text)
    gz.write_bytes(bu.bgzf(text, member_text, 6))
    a = _compress(plain, str(tmp_path / f"{tag}_plain"), L, K, E, p, q)
    b = _compress(gz, str(tmp_path / f"{tag}_bgzf"), L, K, E, p, q)
    assert sorted(a) == sorted(b)
    for f in a:
        assert a[f] == b[f], f
    return a


def _golden_fastq(case):
    g = ol.load_golden(case)
    reads = g["reads.txt"].split()
    L = len(reads[0])
    rng = random.Random(len(reads))
    recs = []
    for i, r in enumerate(reads):
        q = bytes(33 + rng.randrange(2, 41) for _ in range(L))
        recs.append(b"@%s.%d/%d\n%s\n+\n%s\n" % (case.encode(), i, rng.randrange(1000), r, q))
    return b"".join(recs), L


@pytest.mark.parametrize("case", ol.golden_cases())
@pytest.mark.parametrize("member_text", [65280, 4099, 301])
def test_bgzf_and_plain_give_the_same_files_K1(case, member_text, tmp_path):
    text, L = _golden_fastq(case)
    _same_as_plain(tmp_path, text, L, member_text)


@pytest.mark.parametrize("case", ol.golden_cases())
def test_bgzf_K1_E1_matches_the_reference_goldens(case, tmp_path):
    """the stage-II files of a BGZF file are the reference's own (K=1, E=1), byte for byte"""
    import harc_amd
    g = ol.load_golden(case)
    reads = g["reads.txt"].split()
    L = len(reads[0])
    gz = tmp_path / "in.fastq.gz"
    gz.write_bytes(bu.bgzf(b"".join(b"@T.%d some comment\n%s\n+\n%s\n" % (i, r, b"H" * L) for i, r in enumerate(reads)), 4099, 6))
    base = ol.stage_dir(tmp_path, {})
    harc_amd.compress_fastq(str(gz), base, L, num_thr=1, num_chains=1)
    got = ol.read_dir(base)
    assert got["read_order_N.bin"] == g["stage1/read_order_N.bin"] and got["numreads.bin"] == g["stage1/numreads.bin"]
    for f in ol.stage2_files(1):
        assert got[f] == g["stage2/" + f], f


def _big_bgzf_part(args):
    seed, n = args
    import numpy as np
    rs = np.random.RandomState(seed)
    rec = np.empty((n, 218), dtype=np.uint8)
    rec[:, 0] = ord("@"); rec[:, 1:13] = 48 + rs.randint(0, 10, (n, 12)); rec[:, 13] = 10
    rec[:, 14:114] = np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, (n, 100))]
    rec[:, 114] = 10; rec[:, 115] = ord("+"); rec[:, 116] = 10
    rec[:, 117:217] = 35 + rs.randint(0, 38, (n, 100)); rec[:, 217] = 10
    text = rec.tobytes()
    return text, bu.bgzf(text, 65280, 1, eof=False)


def test_large_bgzf_in_pieces_of_64_mb_gives_the_same_files(tmp_path, monkeypatch):
    """more than 200 MB of BGZF in pieces of 64 MB (the feeder's slice size): pieces span slices and overlap the next by 64 KiB, the candidate
    scans run over ~16 000 tiles, the text is carried from piece to piece"""
    import multiprocessing as mp
    with mp.get_context("spawn").Pool(8) as p:                    # fresh interpreters that never open the GPU
        parts = p.map(_big_bgzf_part, [(100 + k, 125000) for k in range(16)])
    text = b"".join(t for t, _ in parts)
    blob = b"".join(b for _, b in parts) + bu.EOF_MARKER
    chunk = 64 << 20
    assert len(blob) >= 200e6 and len(blob) > 3 * chunk
    plain, gz = tmp_path / "big.fastq", tmp_path / "big.fastq.gz"
    plain.write_bytes(text); gz.write_bytes(blob)
    del text, blob, parts
    monkeypatch.setenv("HARC_AMD_INGEST_CHUNK", str(chunk))
    a = _compress(plain, str(tmp_path / "plain"), 100, 0, 4)
    b = _compress(gz, str(tmp_path / "bgzf"), 100, 0, 4)
    assert sorted(a) == sorted(b)
    for f in a:
        assert a[f] == b[f], f
    assert len(a["read_order_N.bin"]) == 0 and int.from_bytes(a["numreads.bin"], "little") == 2000000


@pytest.mark.parametrize("case", ol.golden_cases()[:4])
def test_bgzf_and_plain_give_the_same_files_K4_E2_pq(case, tmp_path, monkeypatch):
    text, L = _golden_fastq(case)
    monkeypatch.setenv("HARC_AMD_INGEST_CHUNK", "50000")          # many pieces, members cut by them
    a = _same_as_plain(tmp_path, text, L, 4099, K=4, E=2, p=True, q=True)
    assert "output.quality" in a and "output.id" in a


@pytest.mark.parametrize("stream,chunk", [("0", "30011"), ("1", "30011"), ("0", "eof"), ("1", "eof")])
def test_bgzf_q_without_p_in_hbm_and_streamed(stream, chunk, tmp_path, monkeypatch):
    """chunk "eof": the last piece owns nothing but bgzip's 28-byte EOF marker, so it holds no text at all"""
    text = bu.fastq_text(4000, 100, seed=21, n_rate=0.01)
    if chunk == "eof":
        chunk = str(len(bu.bgzf(text, 4099, 6)) - 28)
    monkeypatch.setenv("HARC_AMD_Q_STREAM", stream)
    monkeypatch.setenv("HARC_AMD_INGEST_CHUNK", chunk)
    monkeypatch.setenv("HARC_AMD_Q_BIN", "70000")
    a = _same_as_plain(tmp_path, text, 100, 4099, K=4, E=2, q=True)
    assert len(a["output.quality"]) == 4000 * 101


@pytest.mark.parametrize("chunk", [None, "7000"])
def test_bgzf_edge_cases(chunk, tmp_path, monkeypatch):
    if chunk:
        monkeypatch.setenv("HARC_AMD_INGEST_CHUNK", chunk)
    base = bu.fastq_text(1500, 100, seed=4)
    _same_as_plain(tmp_path, base + b"@cut\n" + b"ACGT" * 25, 100, 301, tag="trunc")           # truncated last record: its read counts
    longid = bu.fastq_text(200, 100, seed=6) + bu.fastq_text(1, 100, seed=7, id_len=150000) + bu.fastq_text(300, 100, seed=8)
    _same_as_plain(tmp_path, longid, 100, 4099, p=True, q=True, tag="longid")              # an id line longer than two members
    _same_as_plain(tmp_path, bu.fastq_text(900, 100, seed=5, crlf=True), 100, 4099, tag="crlf")


def test_set_fastq_bgzf_device_equals_set_fastq_device():
    import harc_amd
    text = bu.fastq_text(6000, 100, seed=12, n_rate=0.005)
    blob = bu.bgzf(text, 4099, 6)
    res = []
    for kind in ("plain", "bgzf"):
        with harc_amd.HarcAmd(harc_amd.default_params(100, num_thr=2, num_chains=8, num_steps=16)) as h:
            if kind == "plain":
                d = _dev(text); nrec = h.set_fastq_device(d.data_ptr(), len(text))
            else:
                d = _dev(blob); nrec = h.set_fastq_bgzf_device(d.data_ptr(), len(blob))
            sig = h.input_signature()
            order_n = h.stream("IN_ORDER_N")
            h.reorder(); h.encode()
            res.append((nrec, sig, order_n, [h.stream(s, e) for s in ("S2_SEQ", "S2_POS", "S2_NOISE", "S2_REV") for e in range(2)], h.stream("S2_ORDER")))
    assert res[0] == res[1] and res[0][0] == 6000


def test_corrupt_input_is_refused_naming_the_member(ctx, tmp_path):
    import harc_amd
    text = bu.fastq_text(400, 100, seed=2)
    good = bu.bgzf(text, 4099, 6, eof=False)
    ms = bu.members(good)
    k = 3
    at, size = ms[k]
    m = good[at:at + size]
    chunk = text[k * 4099:(k + 1) * 4099]
    bad_crc = good[:at] + bu.member(chunk, crc=zlib.crc32(chunk) ^ 1) + good[at + size:]
    trunc_last = good[:-5]
    past_end = good[:at] + m[:-1]                                 # BSIZE of the last member points one byte past the end
    big_isize = good[:at] + bu.member(chunk, isize=70000) + good[at + size:]
    for blob, where in [(bad_crc, at), (trunc_last, ms[-1][0]), (past_end, at), (big_isize, at)]:
        with pytest.raises(harc_amd.HarcAmdError) as e:
            _inflate(ctx, blob)
        assert e.value.code == -1 and str(where) in str(e.value), str(e.value)
    assert _inflate(ctx, good) == text                            # the context still works
    gz = tmp_path / "bad.fastq.gz"
    gz.write_bytes(bad_crc)
    os.makedirs(tmp_path / "output")
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.compress_fastq(str(gz), str(tmp_path), 100)
    assert e.value.code == -1 and str(at) in str(e.value)


@pytest.mark.parametrize("flags", [["-p"], ["-q", "-t", "2"], ["-p", "-q", "-t", "3"]])
def test_harc_cli_on_bgzf_end_to_end(flags, tmp_path):
    """./harc -c x.fastq.gz then ./harc -d: the reads come back (in exact order with -p) and x.quality / x.id equal those of the plain run"""
    import subprocess
    from tests import gen
    reads = gen.reads_text(7, 8000, 100, 60000, err=0.01).split()
    rng = random.Random(4)
    text = b"".join(b"@s.%d/%d\n%s\n+\n%s\n" % (i, i % 3, r, bytes(33 + rng.randrange(2, 41) for _ in range(100))) for i, r in enumerate(reads))
    out = {}
    for kind in ("plain", "bgzf"):
        d = tmp_path / kind
        d.mkdir()
        f = d / ("x.fastq" if kind == "plain" else "x.fastq.gz")
        f.write_bytes(text if kind == "plain" else bu.bgzf(text, 65280, 6))
        r = subprocess.run([os.path.join(ROOT_DIR, "harc"), "-c", str(f)] + flags, cwd=ROOT_DIR, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
        assert (d / "x.harc").exists() and not (d / "output").exists()
        r = subprocess.run([os.path.join(ROOT_DIR, "harc"), "-d", str(d / "x.harc")] + (["-p"] if "-p" in flags else []), cwd=ROOT_DIR,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
        out[kind] = {n: (d / n).read_bytes() for n in ("x.dna.d", "x.quality", "x.id") if (d / n).exists()}
    assert out["plain"] == out["bgzf"]
    dec = out["bgzf"]["x.dna.d"].split()
    assert (dec == reads) if "-p" in flags else (sorted(dec) == sorted(reads))
    if "-q" in flags:
        assert "x.quality" in out["bgzf"] and "x.id" in out["bgzf"]
