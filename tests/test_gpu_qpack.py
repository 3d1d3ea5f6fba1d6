"""The packed quality file on the GPU: harc_amd_qpack_device against the encoder run in a row on the host (the same bytes, whatever the alignment, nothing
written outside them), harc_amd_qunpack_device back and on damaged input, the stride check, the two file calls in small pieces, and ./harc -c -q -Q / -d -q end
to end."""
import gzip
import os
import subprocess

import pytest

from tests import gen
from tests import quality_cases as qc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
CASES = qc.small_cases()
_HOST = {}


def _host(name):
    """the host twin's file for a case, computed once"""
    import harc_amd
    if name not in _HOST:
        text, L, rb = CASES[name]
        _HOST[name] = harc_amd.qpack_host(text, L, rb)
    return _HOST[name]


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


def _pack(h, text, L, rb, in_off=3, out_off=0, header=True, cap=None):
    """-> the bytes written; the guard bytes either side of them must stay 0xEE"""
    import harc_amd
    import torch
    n = len(text) // (L + 1)
    tt, pt = _dev(text, in_off)
    bound = harc_amd.qpack_bound(n, L, rb)
    out = torch.full((bound + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    at = 16 + out_off
    torch.cuda.synchronize()                                      # the library works on a stream of its own
    got = h.qpack_device(pt, n, L, rb, out.data_ptr() + at, bound if cap is None else cap, header=header)
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    assert host[:at] == b"\xee" * at and host[at + got:] == b"\xee" * (len(host) - at - got), "bytes outside the output were written"
    return host[at:at + got]


def _unpack(h, blob, in_off=5, out_off=7):
    import torch
    tb, pb = _dev(blob, in_off)
    torch.cuda.synchronize()
    size = h.qunpack_device(pb, len(blob))
    out = torch.full((size + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    at = 16 + out_off
    torch.cuda.synchronize()
    assert h.qunpack_device(pb, len(blob), out.data_ptr() + at, size) == size
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    assert host[:at] == b"\xee" * at and host[at + size:] == b"\xee" * (len(host) - at - size), "bytes outside the text were written"
    return host[at:at + size]


@pytest.mark.parametrize("out_off", [0, 9])
@pytest.mark.parametrize("in_off", [1, 3, 5])
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_pack_writes_the_host_bytes_and_unpacks_to_the_text(ctx, name, in_off, out_off):
    import harc_amd
    text, L, rb = CASES[name]
    header = out_off == 0 or len(text) % 2 == 0                   # with and without the file header over the cases
    blob = _pack(ctx, text, L, rb, in_off=in_off, out_off=out_off, header=header)
    want = _host(name)
    assert blob == (want if header else want[32:])
    if not header:
        blob = want[:32] + blob
    assert _unpack(ctx, blob, in_off=in_off, out_off=out_off) == text
    assert harc_amd.qunpack_host(blob) == text


def test_device_pack_size_only_and_capacity_one_byte_short(ctx):
    import harc_amd
    import torch
    text, L, rb = CASES["cut_901_RB300"]
    n = len(text) // (L + 1)
    tt, pt = _dev(text, 3)
    torch.cuda.synchronize()
    size = ctx.qpack_device(pt, n, L, rb)                          # no output: the size alone
    assert size == len(_host("cut_901_RB300"))
    out = torch.zeros(size + 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(harc_amd.HarcAmdError) as e:
        ctx.qpack_device(pt, n, L, rb, out.data_ptr(), size - 1)
    assert e.value.code == EINVAL and str(size) in str(e.value) and str(size - 1) in str(e.value), str(e.value)
    assert ctx.qpack_device(pt, n, L, rb, out.data_ptr(), size) == size
    assert out[:size].cpu().numpy().tobytes() == _host("cut_901_RB300")
    # ... and of the unpacked text
    tb, pb = _dev(_host("cut_901_RB300"), 1)
    torch.cuda.synchronize()
    with pytest.raises(harc_amd.HarcAmdError) as e:
        ctx.qunpack_device(pb, size, out.data_ptr(), len(text) - 1)
    assert e.value.code == EINVAL and str(len(text)) in str(e.value) and str(len(text) - 1) in str(e.value), str(e.value)


@pytest.mark.parametrize("which", ["flip_00", "row_sum_plus_1", "strand_length_plus_1", "truncated_tail", "mode_2", "A_+1"])
def test_device_unpack_refuses_damaged_input_and_the_context_goes_on(ctx, which):
    """the damaged files are those that the sanitizer build of the host test handled cleanly"""
    import harc_amd
    import torch
    text = qc.corruption_text()
    packed = harc_amd.qpack_host(text, 100)
    bad = qc.corrupted(packed)[which]
    with pytest.raises(harc_amd.HarcAmdError):
        harc_amd.qunpack_host(bad)                                 # (the flip is one that the host refuses)
    tb, pb = _dev(bad, 5)
    out = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(harc_amd.HarcAmdError) as e:
        ctx.qunpack_device(pb, len(bad), out.data_ptr(), len(text))
    assert e.value.code == EINVAL and "block 0" in str(e.value) and "byte 32" in str(e.value), str(e.value)
    assert _unpack(ctx, packed) == text                            # the call after it on the same context


def test_stride_violations_in_the_text_are_refused_with_counts(ctx):
    import harc_amd
    import torch
    text, L, rb = CASES["L100_700"]
    n = len(text) // (L + 1)
    for at, byte, counts in ((300 * 101 + 40, 10, "0 positions on the 101-byte stride hold no newline and 1 newlines"),
                             (300 * 101 + 100, ord("I"), "1 positions on the 101-byte stride hold no newline and 0 newlines")):
        b = bytearray(text)
        b[at] = byte
        tt, pt = _dev(bytes(b), 3)
        torch.cuda.synchronize()
        with pytest.raises(harc_amd.HarcAmdError) as e:
            ctx.qpack_device(pt, n, L, rb)
        assert e.value.code == EINVAL and counts in str(e.value), str(e.value)
        with pytest.raises(harc_amd.HarcAmdError) as e:
            harc_amd.qpack_host(bytes(b), L, rb)
        assert e.value.code == EINVAL and counts in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------------ the file calls
def test_file_calls_are_a_function_of_the_text_and_the_block_size_alone(tmp_path, monkeypatch, capfd):
    import harc_amd
    L, n = 100, 5000
    text = qc.markov(n, L, seed=21)
    q = tmp_path / "x.quality"
    q.write_bytes(text)
    want = harc_amd.qpack_host(text, L, 300)
    monkeypatch.setenv("HARC_AMD_QPACK_BLOCK", "300")
    monkeypatch.setenv("HARC_AMD_FEED_SLICE", "256")
    for piece in ("1", "2", "64"):
        monkeypatch.setenv("HARC_AMD_QPACK_PIECE", piece)
        monkeypatch.setenv("HARC_AMD_TRACE", "1")
        out = tmp_path / ("x.%s.hq" % piece)
        harc_amd.qpack_files(str(q), str(out))
        line = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[qpack]")]
        monkeypatch.delenv("HARC_AMD_TRACE")
        assert out.read_bytes() == want, piece
        assert len(line) == 1 and "%d bytes of text -> %d bytes in 17 blocks (0 stored), %d pieces" % (len(text), len(want), (17 + int(piece) - 1) // int(piece)) in line[0], line
        back = tmp_path / ("x.%s.back" % piece)
        harc_amd.qunpack_files(str(out), str(back))
        assert back.read_bytes() == text, piece
    # refusals leave no output
    out = tmp_path / "bad.hq"
    q.write_bytes(text[:-7])
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.qpack_files(str(q), str(out))
    assert e.value.code == EINVAL and not out.exists()
    (tmp_path / "cut.hq").write_bytes(want[:-9])
    back = tmp_path / "cut.back"
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.qunpack_files(str(tmp_path / "cut.hq"), str(back))
    assert e.value.code == EINVAL and not back.exists()
    monkeypatch.delenv("HARC_AMD_QPACK_BLOCK")
    (tmp_path / "e.quality").write_bytes(b"")
    harc_amd.qpack_files(str(tmp_path / "e.quality"), str(tmp_path / "e.hq"))
    assert (tmp_path / "e.hq").read_bytes() == harc_amd.qpack_host(b"", 100)
    harc_amd.qunpack_files(str(tmp_path / "e.hq"), str(tmp_path / "e.back"))
    assert (tmp_path / "e.back").read_bytes() == b""


def test_a_damaged_block_of_a_later_piece_is_named_by_its_number_and_byte_in_the_file(tmp_path, monkeypatch):
    """three blocks in three pieces, the mode byte of the last set to 2 (refused by rule): the file call and the host twin name block 2 and its byte in the file"""
    import harc_amd
    text = qc.markov(700, 100, seed=5)
    bad = bytearray(harc_amd.qpack_host(text, 100, 300))
    off, at = [], 32                                               # the blocks behind the 32-byte header, by their u32 payload sizes
    while at < len(bad):
        off.append(at)
        at += 4 + int.from_bytes(bad[at:at + 4], "little")
    assert at == len(bad) and len(off) == 3
    bad[off[2] + 4] = 2                                            # the first byte of the payload
    monkeypatch.setenv("HARC_AMD_QPACK_BLOCK", "300")
    monkeypatch.setenv("HARC_AMD_QPACK_PIECE", "1")
    monkeypatch.setenv("HARC_AMD_FEED_SLICE", "256")
    (tmp_path / "bad.packed").write_bytes(bytes(bad))
    back = tmp_path / "bad.back"
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.qunpack_files(str(tmp_path / "bad.packed"), str(back))
    with pytest.raises(harc_amd.HarcAmdError) as eh:
        harc_amd.qunpack_host(bytes(bad))
    for err in (e.value, eh.value):
        assert err.code == EINVAL and "block 2 " in str(err) and "byte %d " % off[2] in str(err) and "is damaged" in str(err), str(err)
    assert not back.exists()


# ------------------------------------------------------------------------------------------------ ./harc
def _harc(args, env):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _join(ids, reads, quals):
    return b"".join(b"%s\n%s\n+\n%s\n" % t for t in zip(ids, reads, quals))


@pytest.mark.parametrize("flags", [["-p"], [], ["-p", "-z"]])
def test_harc_packs_the_quality_values_and_restores_the_fastq(tmp_path, flags):
    import harc_amd
    L, n = 100, 3000
    order = [f for f in flags if f == "-p"]
    # without -p the reference's .id file pairs ids with reads only on inputs without N (README): such a run gets none
    reads = gen.reads_text(31, n, L, 20000, err=0.01, n_frac=0.25 if order else 0.0).split()
    quals = qc.markov(len(reads), L, seed=17).split()
    ids = [b"@run7.%d len=%d/%d" % (i, L, 1 + i % 2) for i in range(len(reads))]
    fq = tmp_path / "x.fastq"
    fq.write_bytes(_join(ids, reads, quals))
    env = dict(os.environ, HARC_AMD_STAGE3="none")
    r = _harc(["-c", str(fq)] + order + ["-q", "-Q", "-t", "2"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    hq = tmp_path / "x.quality.hq"
    assert hq.exists() and not (tmp_path / "x.quality").exists() and not (tmp_path / "output").exists()
    packed = hq.read_bytes()
    qtext = harc_amd.qunpack_host(packed)
    assert len(packed) < len(qtext) // 2 and packed == harc_amd.qpack_host(qtext, L)
    r = _harc(["-d", str(tmp_path / "x.harc")] + flags + ["-q"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert not (tmp_path / "output").exists() and hq.exists()
    got = gzip.decompress((tmp_path / "x.d.fastq.gz").read_bytes()) if "-z" in flags else (tmp_path / "x.d.fastq").read_bytes()
    if order:
        assert got == fq.read_bytes()
    else:                                                          # reordered: the quality lines still pair with their reads
        rec = got.split(b"\n")
        pairs = sorted(zip(rec[1::4], rec[3::4]))
        assert pairs == sorted(zip(reads, quals)) and sorted(qtext.split()) == sorted(quals)
