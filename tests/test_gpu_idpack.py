"""The packed id file on the GPU: harc_amd_idpack_device against the encoder run in a row on the host (the same bytes, whatever the alignment, nothing written
outside them), harc_amd_idunpack_device back and on damaged input, the missing final newline, the two file calls in small pieces, and ./harc -c -q -I /
-d -q end to end."""
import gzip
import os
import subprocess

import pytest

from tests import gen
from tests import id_cases as ic
from tests import quality_cases as qc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
CASES = ic.small_cases()
_HOST = {}


def _host(name):
    """the host twin's file for a case, computed once"""
    import harc_amd
    if name not in _HOST:
        text, rb = CASES[name]
        _HOST[name] = harc_amd.idpack_host(text, rb)
    return _HOST[name]


@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        yield h


def _dev(b, off):
    """b at a buffer's byte `off`, 0xEE around it -> (tensor, pointer).  The text ends 16 - off bytes in front of the buffer's end: nothing behind it belongs to it"""
    import torch
    t = torch.full((len(b) + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    if b:
        t[off:off + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + off


def _pack(h, text, rb, in_off=3, out_off=0, header=True, cap=None):
    """-> the bytes written; the guard bytes either side of them must stay 0xEE"""
    import harc_amd
    import torch
    tt, pt = _dev(text, in_off)
    bound = harc_amd.idpack_bound(len(text), text.count(b"\n"), rb)
    out = torch.full((bound + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    at = 16 + out_off
    torch.cuda.synchronize()                                      # the library works on a stream of its own
    got = h.idpack_device(pt, len(text), rb, out.data_ptr() + at, bound if cap is None else cap, header=header)
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    assert host[:at] == b"\xee" * at and host[at + got:] == b"\xee" * (len(host) - at - got), "bytes outside the output were written"
    return host[at:at + got]


def _unpack(h, blob, in_off=5, out_off=7):
    import torch
    tb, pb = _dev(blob, in_off)
    torch.cuda.synchronize()
    size = h.idunpack_device(pb, len(blob))
    out = torch.full((size + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    at = 16 + out_off
    torch.cuda.synchronize()
    assert h.idunpack_device(pb, len(blob), out.data_ptr() + at, size) == size
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    assert host[:at] == b"\xee" * at and host[at + size:] == b"\xee" * (len(host) - at - size), "bytes outside the text were written"
    return host[at:at + size]


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_pack_writes_the_host_bytes_and_unpacks_to_the_text(ctx, name):
    """every input misalignment 1, 3, 5 with every output misalignment 0, 9; with and without the file header over them"""
    import harc_amd
    text, rb = CASES[name]
    want = _host(name)
    for in_off in (1, 3, 5):
        for out_off in (0, 9):
            header = (in_off + out_off) % 4 != 0
            blob = _pack(ctx, text, rb, in_off=in_off, out_off=out_off, header=header)
            assert blob == (want if header else want[32:]), (in_off, out_off, header)
            assert _unpack(ctx, want, in_off=in_off, out_off=out_off) == text, (in_off, out_off)
    assert harc_amd.idunpack_host(want) == text


def test_device_pack_size_only_and_capacity_one_byte_short(ctx):
    import harc_amd
    import torch
    text, rb = CASES["cut_901_RB300"]
    want = _host("cut_901_RB300")
    tt, pt = _dev(text, 3)
    torch.cuda.synchronize()
    size = ctx.idpack_device(pt, len(text), rb)                    # no output: the size alone
    assert size == len(want)
    out = torch.zeros(size + 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(harc_amd.HarcAmdError) as e:
        ctx.idpack_device(pt, len(text), rb, out.data_ptr(), size - 1)
    assert e.value.code == EINVAL and str(size) in str(e.value) and str(size - 1) in str(e.value), str(e.value)
    assert ctx.idpack_device(pt, len(text), rb, out.data_ptr(), size) == size
    assert out[:size].cpu().numpy().tobytes() == want
    # ... and of the unpacked text
    tb, pb = _dev(want, 1)
    torch.cuda.synchronize()
    with pytest.raises(harc_amd.HarcAmdError) as e:
        ctx.idunpack_device(pb, size, out.data_ptr(), len(text) - 1)
    assert e.value.code == EINVAL and str(len(text)) in str(e.value) and str(len(text) - 1) in str(e.value), str(e.value)


def test_device_unpack_refuses_every_damaged_input_as_the_host_does_and_the_context_goes_on(ctx):
    """the damaged files are those that the sanitizer build of the host test handled cleanly"""
    import harc_amd
    import torch
    text = ic.corruption_text()
    packed = harc_amd.idpack_host(text)
    bad = ic.corrupted(packed)
    out = torch.full((len(text) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    for which in sorted(bad):
        with pytest.raises(harc_amd.HarcAmdError) as eh:
            harc_amd.idunpack_host(bad[which])
        tb, pb = _dev(bad[which], 5)
        torch.cuda.synchronize()
        with pytest.raises(harc_amd.HarcAmdError) as e:
            ctx.idunpack_device(pb, len(bad[which]), out.data_ptr() + 16, len(text) + 1)
        torch.cuda.synchronize()
        assert e.value.code == eh.value.code == EINVAL, (which, str(e.value))
        if which != "wrong_magic":
            assert "block 0" in str(e.value) and "block 0" in str(eh.value), (which, str(e.value), str(eh.value))
        if "is damaged" in str(eh.value) and "is damaged" in str(e.value):       # both came as far as the block: the same block, byte and reason
            assert str(e.value).split("idunpack: ")[1] == str(eh.value).split("idunpack: ")[1], (which, str(e.value), str(eh.value))
    host = out.cpu().numpy().tobytes()
    assert host[:16] == b"\xee" * 16 and host[16 + len(text):] == b"\xee" * 48, "bytes outside the text were written"
    assert _unpack(ctx, packed) == text                            # the call after them on the same context


def test_a_missing_final_newline_is_refused(ctx):
    import harc_amd
    import torch
    text = CASES["m_257"][0][:-1]
    tt, pt = _dev(text, 3)
    torch.cuda.synchronize()
    with pytest.raises(harc_amd.HarcAmdError) as e:
        ctx.idpack_device(pt, len(text), 0)
    assert e.value.code == EINVAL and "newline" in str(e.value), str(e.value)
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.idpack_host(text)
    assert e.value.code == EINVAL and "newline" in str(e.value), str(e.value)
    assert ctx.idpack_device(0, 0, 0) == 32                        # the empty text: the header alone


# ------------------------------------------------------------------------------------------------ the file calls
def test_file_calls_are_a_function_of_the_text_and_the_block_size_alone(tmp_path, monkeypatch, capfd):
    import harc_amd
    lines = list(ic.illumina_ids()[:5000])
    lines[1234] = b"@long " + b"xyz" * 9000                         # a line longer than a piece of the ring
    text = ic.text(lines)
    p = tmp_path / "x.id"
    p.write_bytes(text)
    want = harc_amd.idpack_host(text, 300)
    monkeypatch.setenv("HARC_AMD_IDPACK_BLOCK", "300")
    monkeypatch.setenv("HARC_AMD_FEED_SLICE", "4096")             # a ring of a few records
    for piece in ("1", "2", "8"):
        monkeypatch.setenv("HARC_AMD_IDPACK_PIECE", piece)
        monkeypatch.setenv("HARC_AMD_TRACE", "1")
        out = tmp_path / ("x.%s.hi" % piece)
        harc_amd.idpack_files(str(p), str(out))
        line = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[idpack]")]
        monkeypatch.delenv("HARC_AMD_TRACE")
        assert out.read_bytes() == want, piece
        assert len(line) == 1 and "%d bytes of text -> %d bytes in 17 blocks (" % (len(text), len(want)) in line[0] and " pieces: " in line[0], line
        back = tmp_path / ("x.%s.back" % piece)
        harc_amd.idunpack_files(str(out), str(back))
        assert back.read_bytes() == text, piece
    # long ids: a call of 8 blocks is cut by the line index to the text it may hold, down to a block a call; the same file
    monkeypatch.setenv("HARC_AMD_IDPACK_CALL_TEXT", "30000")
    monkeypatch.setenv("HARC_AMD_TRACE", "1")
    out = tmp_path / "x.cut.hi"
    harc_amd.idpack_files(str(p), str(out))
    line = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[idpack]")]
    monkeypatch.delenv("HARC_AMD_TRACE")
    monkeypatch.delenv("HARC_AMD_IDPACK_CALL_TEXT")
    assert out.read_bytes() == want and len(line) == 1 and "in 17 blocks (" in line[0] and ", 17 pieces: " in line[0], line
    # refusals leave no output
    out = tmp_path / "bad.hi"
    p.write_bytes(text[:-1])
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.idpack_files(str(p), str(out))
    assert e.value.code == EINVAL and "newline" in str(e.value) and not out.exists()
    (tmp_path / "cut.hi").write_bytes(want[:-9])
    back = tmp_path / "cut.back"
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.idunpack_files(str(tmp_path / "cut.hi"), str(back))
    assert e.value.code == EINVAL and not back.exists()
    monkeypatch.delenv("HARC_AMD_IDPACK_BLOCK")
    (tmp_path / "e.id").write_bytes(b"")
    harc_amd.idpack_files(str(tmp_path / "e.id"), str(tmp_path / "e.hi"))
    assert (tmp_path / "e.hi").read_bytes() == harc_amd.idpack_host(b"")
    harc_amd.idunpack_files(str(tmp_path / "e.hi"), str(tmp_path / "e.back"))
    assert (tmp_path / "e.back").read_bytes() == b""


def test_a_damaged_block_of_a_later_piece_is_named_by_its_number_and_byte_in_the_file(tmp_path, monkeypatch):
    """three blocks in three pieces, the mode byte of the last set to 2 (refused by rule): the file call and the host twin name block 2 and its byte in the file"""
    import harc_amd
    text = ic.text(list(ic.illumina_ids()[:700]))
    bad = bytearray(harc_amd.idpack_host(text, 300))
    off, at = [], 32                                               # the blocks behind the 32-byte header, by their u32 payload sizes
    while at < len(bad):
        off.append(at)
        at += 4 + int.from_bytes(bad[at:at + 4], "little")
    assert at == len(bad) and len(off) == 3
    bad[off[2] + 4] = 2                                            # the first byte of the payload
    monkeypatch.setenv("HARC_AMD_IDPACK_BLOCK", "300")
    monkeypatch.setenv("HARC_AMD_IDPACK_PIECE", "1")
    monkeypatch.setenv("HARC_AMD_FEED_SLICE", "4096")
    (tmp_path / "bad.packed").write_bytes(bytes(bad))
    back = tmp_path / "bad.back"
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.idunpack_files(str(tmp_path / "bad.packed"), str(back))
    with pytest.raises(harc_amd.HarcAmdError) as eh:
        harc_amd.idunpack_host(bytes(bad))
    for err in (e.value, eh.value):
        assert err.code == EINVAL and "block 2 " in str(err) and "byte %d " % off[2] in str(err) and "is damaged" in str(err), str(err)
    assert not back.exists()


# ------------------------------------------------------------------------------------------------ ./harc
def _harc(args, env):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _join(ids, reads, quals):
    return b"".join(b"%s\n%s\n+\n%s\n" % t for t in zip(ids, reads, quals))


@pytest.mark.parametrize("flags", [["-p", "-Q"], ["-p", "-Q", "-z"], ["-p"]])
def test_harc_packs_the_ids_and_restores_the_fastq(tmp_path, flags):
    import harc_amd
    L, n = 100, 3000
    reads = gen.reads_text(31, n, L, 20000, err=0.01, n_frac=0.25).split()
    quals = qc.markov(len(reads), L, seed=17).split()
    ids = list(ic.illumina_ids()[:len(reads)])
    fq = tmp_path / "x.fastq"
    fq.write_bytes(_join(ids, reads, quals))
    env = dict(os.environ, HARC_AMD_STAGE3="none")
    pack = [f for f in flags if f == "-Q"]
    r = _harc(["-c", str(fq), "-p", "-q", "-I", "-t", "2"] + pack, env)
    assert r.returncode == 0, r.stdout[-2000:]
    hi = tmp_path / "x.id.hi"
    assert hi.exists() and not (tmp_path / "x.id").exists() and not (tmp_path / "output").exists()
    if pack:
        assert (tmp_path / "x.quality.hq").exists() and not (tmp_path / "x.quality").exists()
    else:                                                          # -I alone leaves the quality values as text
        assert (tmp_path / "x.quality").read_bytes() == ic.text(quals) and not (tmp_path / "x.quality.hq").exists()
    packed = hi.read_bytes()
    assert harc_amd.idunpack_host(packed) == ic.text(ids) and packed == harc_amd.idpack_host(ic.text(ids)) and len(packed) < len(ic.text(ids)) // 4
    r = _harc(["-d", str(tmp_path / "x.harc"), "-q"] + [f for f in flags if f != "-Q"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert not (tmp_path / "output").exists() and hi.exists()
    got = gzip.decompress((tmp_path / "x.d.fastq.gz").read_bytes()) if "-z" in flags else (tmp_path / "x.d.fastq").read_bytes()
    assert got == fq.read_bytes()
