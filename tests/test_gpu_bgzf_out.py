"""BGZF output on the GPU: harc_amd_bgzf_deflate_device against gzip, against the library's own inflate kernel and against the encoder run in a row on the
host (the same bytes); its size against zlib level 1; harc_amd_fastq_assemble_files_ex with bgzf; and ./harc -c -q, -d -q -z, -c of the .gz end to end."""
import gzip
import os
import random
import subprocess

import pytest

from tests import bgzf_out_cases as cases
from tests import bgzf_util as bu
from tests import gen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
TEXTS = cases.texts()


@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        yield h


def _dev(b, off):
    import torch
    t = torch.zeros(len(b) + off + 32, dtype=torch.uint8, device="cuda")
    if b:
        t[off:off + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + off


def _deflate(h, text, in_off=3, out_off=0, eof=True, cap=None):
    """-> the bytes written; the guard bytes either side of them must stay 0xEE"""
    import harc_amd
    import torch
    tt, pt = _dev(text, in_off)
    bound = harc_amd.bgzf_bound(len(text))
    out = torch.full((bound + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    at = 16 + out_off
    torch.cuda.synchronize()                                      # the library works on a stream of its own
    n = h.bgzf_deflate_device(pt, len(text), out.data_ptr() + at, bound if cap is None else cap, eof=eof)
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    assert host[:at] == b"\xee" * at and host[at + n:] == b"\xee" * (len(host) - at - n), "bytes outside the output were written"
    return host[at:at + n]


def _inflate(h, blob):
    import torch
    tb, pb = _dev(blob, 5)
    torch.cuda.synchronize()
    size = h.bgzf_inflate_device(pb, len(blob))
    out = torch.zeros(size + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert h.bgzf_inflate_device(pb, len(blob), out.data_ptr(), size) == size
    torch.cuda.synchronize()
    return out[:size].cpu().numpy().tobytes()


def _check(h, text, blob, eof):
    import harc_amd
    assert (gzip.decompress(blob) if blob else b"") == text
    ms = bu.members(blob)
    sizes = [int.from_bytes(blob[o + s - 4:o + s], "little") for o, s in ms]
    nm = (len(text) + cases.MEMBER - 1) // cases.MEMBER
    assert len(ms) == nm + (1 if eof else 0)
    assert sizes[:nm] == [cases.MEMBER] * (nm - 1) + ([len(text) - (nm - 1) * cases.MEMBER] if nm else [])
    assert all(s <= 65536 for _, s in ms)
    assert blob.endswith(bu.EOF_MARKER) == eof
    if eof:
        assert sizes[-1] == 0 and ms[-1][1] == 28
    assert _inflate(h, blob) == text                              # what ./harc -c reads
    assert blob == harc_amd.bgzf_deflate_host(text, eof=eof)       # the kernels and the encoder in a row write the same bytes
    assert len(blob) <= harc_amd.bgzf_bound(len(text))


@pytest.mark.parametrize("out_off", [0, 9])
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_device_call_writes_bgzf_that_gzip_and_the_inflate_kernel_read(ctx, name, out_off):
    text = TEXTS[name]
    eof = out_off == 0 or len(text) % 2 == 0                      # with and without the marker over the texts
    blob = _deflate(ctx, text, in_off=1 + 2 * (len(text) % 3), out_off=out_off, eof=eof)
    _check(ctx, text, blob, eof)


def test_device_call_members_are_what_they_are_meant_to_be(ctx):
    stored = _deflate(ctx, TEXTS["random_70000"], eof=False)
    assert len(stored) == 70000 + 2 * 31                           # two stored members
    assert _deflate(ctx, b"", eof=True) == bu.EOF_MARKER and _deflate(ctx, b"", eof=False) == b""
    assert len(_deflate(ctx, TEXTS["identical_300_L255"], eof=False)) < 3000
    assert len(_deflate(ctx, TEXTS["newlines_1000"], eof=False)) < 100


def test_device_call_capacity_one_byte_short_is_refused_with_both_sizes(ctx):
    import harc_amd
    import torch
    text = TEXTS["fastq_cut_65281"]
    tt, pt = _dev(text, 3)
    torch.cuda.synchronize()
    size = ctx.bgzf_deflate_device(pt, len(text))                  # no output: the size alone
    assert size == len(harc_amd.bgzf_deflate_host(text))
    out = torch.zeros(size + 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(harc_amd.HarcAmdError) as e:
        ctx.bgzf_deflate_device(pt, len(text), out.data_ptr(), size - 1)
    assert e.value.code == EINVAL and str(size) in str(e.value) and str(size - 1) in str(e.value), str(e.value)
    assert ctx.bgzf_deflate_device(pt, len(text), out.data_ptr(), size) == size
    assert harc_amd.bgzf_bound(0) == 28 and harc_amd.bgzf_bound(1) == 65311 + 28 and harc_amd.bgzf_bound(65281) == 2 * 65311 + 28


@pytest.mark.parametrize("which", ["illumina", "fastq_text"])
def test_output_is_no_larger_than_zlib_level_1(ctx, which):
    """the record-aligned matcher with one dynamic block per member against bgzip -l 1 with the same cuts (a literal-only encoder is 1.27 x zlib's size on the
    first text)"""
    text = cases.illumina_text(20000) if which == "illumina" else bu.fastq_text(20000, 100, seed=3)
    blob = _deflate(ctx, text)
    assert gzip.decompress(blob) == text
    ref1, ref6 = len(bu.bgzf(text, 65280, level=1)), len(bu.bgzf(text, 65280, level=6))
    print("bgzf_out size %s: %d bytes of text -> %d; zlib level 1 %d (ratio %.4f), level 6 %d (ratio %.4f)" % (which, len(text), len(blob), ref1, len(blob) / ref1, ref6, len(blob) / ref6))
    assert len(blob) <= ref1


# ------------------------------------------------------------------------------------------------ the file call
def _join(ids, reads, quals):
    return b"".join(b"%s\n%s\n+\n%s\n" % t for t in zip(ids, reads, quals))


def _text(lines):
    return b"".join(l + b"\n" for l in lines)


def _records(seed, n, L, idlens=(0, 1, 15, 16, 17, 49)):
    rng = random.Random(seed)
    ids = [bytes(rng.choice(b"@abc.:/ 0123456789") for _ in range(rng.choice(idlens))) for _ in range(n)]
    return ids, [bytes(rng.choice(b"ACGTN") for _ in range(L)) for _ in range(n)], [bytes(rng.choice(b"#5FHJ+@") for _ in range(L)) for _ in range(n)]


def _write_three(d, ids, reads, quals):
    (d / "r.dna").write_bytes(_text(reads))
    (d / "r.id").write_bytes(_text(ids))
    (d / "r.quality").write_bytes(_text(quals))
    return str(d / "r.dna"), str(d / "r.id"), str(d / "r.quality")


@pytest.mark.parametrize("n", [5000, 3])
def test_file_call_is_a_function_of_the_text_alone(n, tmp_path, monkeypatch, capfd):
    import harc_amd
    L = 100
    ids, reads, quals = _records(n, n, L)
    want = _join(ids, reads, quals)
    dna, idf, qf = _write_three(tmp_path, ids, reads, quals)
    monkeypatch.setenv("HARC_AMD_TRACE", "1")
    harc_amd.fastq_assemble(dna, idf, qf, str(tmp_path / "a.gz"), bgzf=True)
    a = (tmp_path / "a.gz").read_bytes()
    line = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[fastq_out]")]
    assert len(line) == 1 and "%d bytes of text -> %d bytes in %d members" % (len(want), len(a), (len(want) + 65279) // 65280) in line[0], line
    monkeypatch.delenv("HARC_AMD_TRACE")
    assert gzip.decompress(a) == want and a.endswith(bu.EOF_MARKER)
    assert a == harc_amd.bgzf_deflate_host(want)                   # the device call over the whole text would write the same file
    monkeypatch.setenv("HARC_AMD_FQOUT_PIECE", "1000")
    monkeypatch.setenv("HARC_AMD_FEED_SLICE", "256")
    harc_amd.fastq_assemble(dna, idf, qf, str(tmp_path / "b.gz"), bgzf=True)
    assert (tmp_path / "b.gz").read_bytes() == a
    # bgzf=False: byte for byte what the plain call writes
    harc_amd.fastq_assemble(dna, idf, qf, str(tmp_path / "c.fastq"), bgzf=False)
    harc_amd.fastq_assemble(dna, idf, qf, str(tmp_path / "d.fastq"))
    assert (tmp_path / "c.fastq").read_bytes() == (tmp_path / "d.fastq").read_bytes() == want


def test_file_call_growing_piece_and_empty_inputs(tmp_path, monkeypatch):
    import harc_amd
    n, L = 3000, 100
    ids, reads, quals = _records(8, n, L)
    ids[n // 2] = b"@" + b"w" * 299                                # a piece of 64 bytes has to grow until it holds this line
    dna, idf, qf = _write_three(tmp_path, ids, reads, quals)
    harc_amd.fastq_assemble(dna, idf, qf, str(tmp_path / "a.gz"), bgzf=True)
    monkeypatch.setenv("HARC_AMD_FQOUT_PIECE", "64")
    harc_amd.fastq_assemble(dna, idf, qf, str(tmp_path / "b.gz"), bgzf=True)
    b = (tmp_path / "b.gz").read_bytes()
    assert gzip.decompress(b) == _join(ids, reads, quals) and b == (tmp_path / "a.gz").read_bytes()
    for f in (dna, idf, qf):
        open(f, "wb").close()
    harc_amd.fastq_assemble(dna, idf, qf, str(tmp_path / "e.gz"), bgzf=True)
    assert (tmp_path / "e.gz").read_bytes() == bu.EOF_MARKER


def test_file_call_refusals_leave_no_output(tmp_path):
    import harc_amd
    L, n = 100, 500
    ids, reads, quals = _records(4, n, L)
    dna, idf, qf = _write_three(tmp_path, ids, reads, quals)
    out = str(tmp_path / "r.fastq.gz")
    open(idf, "wb").write(_text(ids[:-1]))                         # an id file a line short
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.fastq_assemble(dna, idf, qf, out, bgzf=True)
    assert e.value.code == EINVAL and "499" in str(e.value) and "500" in str(e.value), str(e.value)
    assert not os.path.exists(out)
    open(idf, "wb").write(_text(ids))
    open(qf, "wb").write(_text(quals[:-1]))                        # sizes that disagree
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.fastq_assemble(dna, idf, qf, out, bgzf=True)
    assert e.value.code == EINVAL and not os.path.exists(out)


# ------------------------------------------------------------------------------------------------ ./harc
def _harc(args, env):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _streams(archive, d):
    """every stream file of an archive made with HARC_AMD_STAGE3=none -> {name: bytes}; the shard files inside each <stream>.tar, not the tar itself,
    whose headers carry the time it was packed"""
    import tarfile
    os.makedirs(d)
    with tarfile.open(archive) as tf:
        tf.extractall(d)
    out = {}
    for f in sorted(os.listdir(d)):
        p = os.path.join(d, f)
        if f.endswith(".tar"):
            with tarfile.open(p) as tf:
                for m in tf.getmembers():
                    if m.isfile():
                        out[f + ":" + os.path.basename(m.name)] = tf.extractfile(m).read()
        else:
            out[f] = open(p, "rb").read()
    return out


def test_harc_round_trip_without_gzip_on_the_host(tmp_path):
    import numpy as np
    L, n = 100, 3000
    reads = gen.reads_text(31, n, L, 20000, err=0.01).split()
    rs = np.random.RandomState(8)
    quals = [bytes(40 + int(x) for x in rs.randint(0, 30, L)) for _ in reads]
    ids = [b"@run7.%d len=%d/%d" % (i, L, 1 + i % 2) for i in range(len(reads))]
    fq = tmp_path / "x.fastq"
    fq.write_bytes(_join(ids, reads, quals))
    env = dict(os.environ, HARC_AMD_STAGE3="none")
    r = _harc(["-c", str(fq), "-p", "-q", "-t", "2"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    r = _harc(["-d", str(tmp_path / "x.harc"), "-p", "-q", "-z"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    gz = tmp_path / "x.d.fastq.gz"
    assert gzip.decompress(gz.read_bytes()) == fq.read_bytes()
    assert not (tmp_path / "x.d.fastq").exists() and not (tmp_path / "x.dna.d").exists() and not (tmp_path / "output").exists()
    first = _streams(tmp_path / "x.harc", tmp_path / "s1")
    side = {f: (tmp_path / f).read_bytes() for f in ("x.id", "x.quality")}
    # and the written file is one that -c reads on the GPU: the same streams as from the plain file
    again = tmp_path / "again"
    again.mkdir()
    os.replace(gz, again / "x.d.fastq.gz")
    r = _harc(["-c", str(again / "x.d.fastq.gz"), "-p", "-q", "-t", "2"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "expanding it on the host" not in r.stdout
    assert _streams(again / "x.d.harc", tmp_path / "s2") == first
    assert {f: (again / f.replace("x.", "x.d.")).read_bytes() for f in side} == side
