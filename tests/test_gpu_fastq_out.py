"""The way back to FASTQ on the GPU: harc_amd_fastq_assemble_device and harc_amd_fastq_assemble_files against the plain Python join of the lines (exact
bytes and sizes, refusals with their counts), the round trip FASTQ -> compress -q -> decode -> assemble through the library (byte for byte with -p, as a
multiset of records without), and ./harc -c -q / -d -q end to end."""
import collections
import json
import os
import random
import subprocess

import pytest

from tests import gen
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _join(ids, reads, quals):
    return b"".join(b"%s\n%s\n+\n%s\n" % t for t in zip(ids, reads, quals))


def _lines(rng, n, L, alphabet):
    return [bytes(rng.choice(alphabet) for _ in range(L)) for _ in range(n)]


def _records(seed, n, L, idlens=(0, 1, 15, 16, 17, 49)):
    rng = random.Random(seed)
    ids = [bytes(rng.choice(b"@abc.:/ 0123456789") for _ in range(rng.choice(idlens))) for _ in range(n)]
    return ids, _lines(rng, n, L, b"ACGTN"), _lines(rng, n, L, b"#5FHJ+@")


def _text(lines):
    return b"".join(l + b"\n" for l in lines)


def _dev(b, off=0):
    """the bytes in device memory, `off` bytes behind a 16-byte boundary (the tensor is kept alive by the caller)"""
    import torch
    t = torch.zeros(len(b) + off + 32, dtype=torch.uint8, device="cuda")
    if b:
        t[off:off + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + off


def _assemble(h, idtext, dna, qual, n, L, out_off=0, cap_less=0):
    """-> (bytes written, n_out); the 16 bytes either side of the output must stay as they were"""
    import torch
    ti, pi = _dev(idtext, 7)
    td, pd = _dev(dna, 3)
    tq, pq = _dev(qual, 5)
    torch.cuda.synchronize()                                      # the library works on a stream of its own: its inputs must be complete
    size = h.fastq_assemble_device(pi, len(idtext), pd, pq, n, L)                   # d_out == NULL: validate, size only
    out = torch.full((size + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    at = 16 + out_off
    torch.cuda.synchronize()
    got = h.fastq_assemble_device(pi, len(idtext), pd, pq, n, L, out.data_ptr() + at, size - cap_less)
    torch.cuda.synchronize()
    assert got == size
    host = out.cpu().numpy().tobytes()
    assert host[:at] == b"\xee" * at and host[at + size:] == b"\xee" * (len(host) - at - size), "bytes outside the output were written"
    return host[at:at + size], size


@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:     # the call's readlen is independent of the context's
        yield h


@pytest.mark.parametrize("L", [1, 15, 16, 100, 255])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1000])
def test_device_call_equals_the_join(ctx, L, n):
    ids, reads, quals = _records(1000 * L + n, n, L)
    want = _join(ids, reads, quals)
    got, size = _assemble(ctx, _text(ids), _text(reads), _text(quals), n, L, out_off=(L + n) % 16)
    assert size == len(want) == len(_text(ids)) + n * (2 * L + 4)
    assert got == want


@pytest.mark.parametrize("out_off", [0, 9])
def test_device_call_records_longer_than_a_tile(ctx, out_off):
    """an id of 40 000 bytes (more than two tiles of output) in the middle and one as the last record; records that straddle tiles around them"""
    L, n = 100, 300
    ids, reads, quals = _records(77, n, L)
    rng = random.Random(3)
    ids[150] = bytes(rng.choice(b"abcdefghij0123456789") for _ in range(40000))
    ids[n - 1] = bytes(rng.choice(b"klmnopqrst0123456789") for _ in range(40000))
    want = _join(ids, reads, quals)
    got, size = _assemble(ctx, _text(ids), _text(reads), _text(quals), n, L, out_off=out_off)
    assert size == len(want) and got == want


@pytest.mark.parametrize("n", [1, 65])
def test_device_call_id_text_without_final_newline(ctx, n):
    L = 16
    ids, reads, quals = _records(5, n, L, idlens=(1, 15, 16, 17, 49))
    idtext = _text(ids)[:-1]
    got, size = _assemble(ctx, idtext, _text(reads), _text(quals), n, L, out_off=5)
    assert size == len(idtext) + 1 + n * (2 * L + 4)
    assert got == _join(ids, reads, quals)


def _refused(ctx, idtext, dna, qual, n, L, cap_less=0, null_too=True):
    import harc_amd
    import torch
    msgs = []
    if null_too:                                                  # the validating call without an output refuses the same inputs
        ti, pi = _dev(idtext, 7); td, pd = _dev(dna, 3); tq, pq = _dev(qual, 5)
        torch.cuda.synchronize()
        with pytest.raises(harc_amd.HarcAmdError) as e:
            ctx.fastq_assemble_device(pi, len(idtext), pd, pq, n, L)
        assert e.value.code == EINVAL
        msgs.append(str(e.value))
    import torch
    ti, pi = _dev(idtext, 7); td, pd = _dev(dna, 3); tq, pq = _dev(qual, 5)
    size = len(idtext) + n * (2 * L + 4)
    out = torch.zeros(size + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(harc_amd.HarcAmdError) as e:
        ctx.fastq_assemble_device(pi, len(idtext), pd, pq, n, L, out.data_ptr(), size - cap_less)
    assert e.value.code == EINVAL
    msgs.append(str(e.value))
    return msgs


def test_device_call_refusals(ctx):
    L, n = 100, 200
    ids, reads, quals = _records(11, n, L, idlens=(1, 15, 16, 17, 49))
    idt, dna, qual = _text(ids), _text(reads), _text(quals)
    for m in _refused(ctx, _text(ids[:-1]), dna, qual, n, L):                        # one id line too few
        assert "199" in m and "200" in m, m
    for m in _refused(ctx, idt + b"@one more\n", dna, qual, n, L):                    # one too many
        assert "201" in m and "200" in m, m
    # a read line one byte short: from there on every newline of the reads sits off the stride (the buffer keeps its size: a byte of padding at the end)
    short = _text(reads[:100]) + reads[100][:-1] + b"\n" + _text(reads[101:]) + b"A"
    off_stride = sum((b == 10) != (i % (L + 1) == L) for i, b in enumerate(short))    # a newline where none belongs and none where one belongs, per line
    assert off_stride == 2 * (n - 100)
    for m in _refused(ctx, idt, short, qual, n, L):
        assert "%d bytes of the reads" % off_stride in m and " 0 bytes of the quality" in m, m
    swapped = bytearray(qual); swapped[5 * (L + 1) + 7] = 10                          # a newline inside a quality line
    for m in _refused(ctx, idt, dna, bytes(swapped), n, L):
        assert " 0 bytes of the reads" in m and " 1 bytes of the quality" in m, m
    size = len(idt) + n * (2 * L + 4)
    for m in _refused(ctx, idt, dna, qual, n, L, cap_less=1, null_too=False):         # capacity one byte too small
        assert str(size) in m and str(size - 1) in m, m
    # and the same inputs are accepted when nothing is wrong
    got, _ = _assemble(ctx, idt, dna, qual, n, L)
    assert got == _join(ids, reads, quals)


# ------------------------------------------------------------------------------------------------ the file call
def _write_three(d, ids, reads, quals, final_newline=True):
    (d / "r.dna").write_bytes(_text(reads))
    (d / "r.id").write_bytes(_text(ids) if final_newline else _text(ids)[:-1])
    (d / "r.quality").write_bytes(_text(quals))
    return str(d / "r.dna"), str(d / "r.id"), str(d / "r.quality"), str(d / "r.fastq")


def _pieces_traced(err):
    lines = [l for l in err.splitlines() if l.startswith("[fastq_out]")]
    assert len(lines) == 1, err[-2000:]
    return int(lines[0].split(" pieces")[0].split()[-1])


@pytest.mark.parametrize("n", [5000, 3])
@pytest.mark.parametrize("mode", ["default", "small_pieces", "growing_piece"])
def test_file_call_equals_the_join(n, mode, tmp_path, monkeypatch, capfd):
    import harc_amd
    L = 100
    ids, reads, quals = _records(n, n, L, idlens=(0, 1, 15, 16, 17, 49))
    if mode == "small_pieces":                                    # many pieces, several slices per piece, partial lines carried
        monkeypatch.setenv("HARC_AMD_FQOUT_PIECE", "1000")
        monkeypatch.setenv("HARC_AMD_FEED_SLICE", "256")
    elif mode == "growing_piece":                                 # an id line of 300 bytes: a piece of 64 has to grow until it holds it
        monkeypatch.setenv("HARC_AMD_FQOUT_PIECE", "64")
        ids[n // 2] = b"@" + b"w" * 299
    monkeypatch.setenv("HARC_AMD_TRACE", "1")
    dna, idf, qf, out = _write_three(tmp_path, ids, reads, quals)
    harc_amd.fastq_assemble(dna, idf, qf, out)
    assert open(out, "rb").read() == _join(ids, reads, quals)
    npieces = _pieces_traced(capfd.readouterr().err)
    if mode == "default":
        assert npieces == 1
    elif mode == "growing_piece" or len(_text(ids)) > 1000:       # (3 ids are less than one piece of 1000 bytes)
        assert npieces > 1


def test_file_call_id_file_without_final_newline_and_empty_files(tmp_path, monkeypatch):
    import harc_amd
    L = 15
    ids, reads, quals = _records(9, 700, L, idlens=(1, 15, 16, 17, 49))
    monkeypatch.setenv("HARC_AMD_FQOUT_PIECE", "333")
    dna, idf, qf, out = _write_three(tmp_path, ids, reads, quals, final_newline=False)
    harc_amd.fastq_assemble(dna, idf, qf, out)
    assert open(out, "rb").read() == _join(ids, reads, quals)
    for f in (dna, idf, qf):
        open(f, "wb").close()
    harc_amd.fastq_assemble(dna, idf, qf, out)
    assert open(out, "rb").read() == b""


def test_file_call_refusals_leave_no_output(tmp_path, monkeypatch):
    import harc_amd
    L, n = 100, 500
    ids, reads, quals = _records(4, n, L)
    dna, idf, qf, out = _write_three(tmp_path, ids, reads, quals)
    open(qf, "wb").write(_text(quals[:-1]))                       # a quality file one line short
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.fastq_assemble(dna, idf, qf, out)
    assert e.value.code == EINVAL and not os.path.exists(out)
    open(qf, "wb").write(_text(quals))
    for piece in (None, "700"):                                   # an id file one line short, seen at the end of one piece or of many
        if piece:
            monkeypatch.setenv("HARC_AMD_FQOUT_PIECE", piece)
        open(idf, "wb").write(_text(ids[:-1]))
        with pytest.raises(harc_amd.HarcAmdError) as e:
            harc_amd.fastq_assemble(dna, idf, qf, out)
        assert e.value.code == EINVAL and "499" in str(e.value) and "500" in str(e.value), str(e.value)
        assert not os.path.exists(out)
        open(idf, "wb").write(_text(ids + [b"@extra"]))           # and one line too many
        with pytest.raises(harc_amd.HarcAmdError) as e:
            harc_amd.fastq_assemble(dna, idf, qf, out)
        assert e.value.code == EINVAL and "501" in str(e.value) and "500" in str(e.value), str(e.value)
        assert not os.path.exists(out)
    open(idf, "wb").write(_text(ids))
    open(dna, "wb").write(_text(reads)[:-1])                      # size(dna) no multiple of L + 1
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.fastq_assemble(dna, idf, qf, out)
    assert e.value.code == EINVAL and not os.path.exists(out)
    open(dna, "wb").write(b"A" * 300 + b"\n")                     # a first line of more than 255 characters
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.fastq_assemble(dna, idf, qf, out)
    assert e.value.code == EINVAL and "255" in str(e.value)


# ------------------------------------------------------------------------------------------------ round trip through the library
CASE = "q_L100_lastN_1500"


def _fixture():
    g = ol.load_golden(CASE)
    return g["in.fastq"], json.loads(g["meta.json"])["L"]


def _four(fq):
    ls = fq.split(b"\n")
    assert ls[-1] == b""
    return [tuple(ls[i:i + 4]) for i in range(0, len(ls) - 1, 4)]


def _roundtrip(d, fq, L, E, po):
    import harc_amd
    os.makedirs(d / "output")
    (d / "in.fastq").write_bytes(fq)
    harc_amd.compress_fastq(str(d / "in.fastq"), str(d), L, num_thr=E, num_chains=4, num_steps=16, preserve_order=po, preserve_quality=True)
    if po:
        harc_amd.pack_order(str(d), L)
    harc_amd.decoder(str(d), E, preserve_order=po)
    od = d / "output"
    harc_amd.fastq_assemble(str(od / "output.dna"), str(od / "output.id"), str(od / "output.quality"), str(d / "out.fastq"))
    return (d / "out.fastq").read_bytes()


@pytest.mark.parametrize("bin_reads", [None, "400"])
def test_roundtrip_preserve_order_gives_the_input_file(bin_reads, tmp_path, monkeypatch):
    fq, L = _fixture()
    assert sum(b"N" in r[1] for r in _four(fq)) == 134
    if bin_reads:
        monkeypatch.setenv("HARC_AMD_BIN_READS", bin_reads)      # the order is restored in several bins
    assert _roundtrip(tmp_path, fq, L, 3, True) == fq


def test_roundtrip_without_preserve_order_keeps_the_records_of_an_input_without_N(tmp_path):
    fq, L = _fixture()
    recs = [r for r in _four(fq) if b"N" not in r[1]]
    assert len(recs) == 1366
    clean = b"".join(b"\n".join(r) + b"\n" for r in recs)
    out = _roundtrip(tmp_path, clean, L, 3, False)
    assert collections.Counter(_four(out)) == collections.Counter(recs)


def test_roundtrip_without_preserve_order_refuses_the_short_id_file(tmp_path):
    """with N reads and without -p the reference's .id file is a line short on this input (its last read has N): the assembler says so, it writes no shifted file"""
    import harc_amd
    fq, L = _fixture()
    with pytest.raises(harc_amd.HarcAmdError) as e:
        _roundtrip(tmp_path, fq, L, 3, False)
    assert e.value.code == EINVAL and "1499" in str(e.value) and "1500" in str(e.value), str(e.value)
    assert not (tmp_path / "out.fastq").exists()


# ------------------------------------------------------------------------------------------------ ./harc
def _harc(args, env):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_harc_c_q_then_d_q_gives_the_fastq_back(tmp_path):
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
    r = _harc(["-d", str(tmp_path / "x.harc"), "-p", "-q"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert (tmp_path / "x.d.fastq").read_bytes() == fq.read_bytes()
    assert not (tmp_path / "x.dna.d").exists() and not (tmp_path / "output").exists()
    r = _harc(["-d", str(tmp_path / "x.harc"), "-p"], env)                          # without -q: as before
    assert r.returncode == 0, r.stdout[-2000:]
    assert (tmp_path / "x.dna.d").read_bytes() == _text(reads)
    assert not (tmp_path / "output").exists()
