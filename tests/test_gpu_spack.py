"""The packed stream file on the GPU: harc_amd_spack_device against the encoder run in a row on the host (the same bytes, whatever the alignment, nothing
written outside them), harc_amd_sunpack_device back and on damaged input of each mode, the two file calls in small pieces, and ./harc -c -S / -d end to end."""
import os
import subprocess
import tarfile

import pytest

from tests import gen
from tests import stream_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
CASES = sc.small_cases()
_HOST = {}


def _host(name):
    """the host twin's file for a case, computed once"""
    import harc_amd
    if name not in _HOST:
        text, B = CASES[name]
        _HOST[name] = harc_amd.spack_host(text, B)
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


def _pack(h, text, B, in_off=3, out_off=0, header=True, cap=None):
    """-> the bytes written; the guard bytes either side of them must stay 0xEE"""
    import harc_amd
    import torch
    tt, pt = _dev(text, in_off)
    bound = harc_amd.spack_bound(len(text), B)
    out = torch.full((bound + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    at = 16 + out_off
    torch.cuda.synchronize()                                      # the library works on a stream of its own
    got = h.spack_device(pt, len(text), B, out.data_ptr() + at, bound if cap is None else cap, header=header)
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    assert host[:at] == b"\xee" * at and host[at + got:] == b"\xee" * (len(host) - at - got), "bytes outside the output were written"
    return host[at:at + got]


def _unpack(h, blob, in_off=5, out_off=7):
    import torch
    tb, pb = _dev(blob, in_off)
    torch.cuda.synchronize()
    size = h.sunpack_device(pb, len(blob))
    out = torch.full((size + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    at = 16 + out_off
    torch.cuda.synchronize()
    assert h.sunpack_device(pb, len(blob), out.data_ptr() + at, size) == size
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    assert host[:at] == b"\xee" * at and host[at + size:] == b"\xee" * (len(host) - at - size), "bytes outside the text were written"
    return host[at:at + size]


def test_the_cases_exercise_every_mode():
    import harc_amd
    sc.check_modes(harc_amd.spack_host)


@pytest.mark.parametrize("out_off", [0, 9])
@pytest.mark.parametrize("in_off", [1, 3, 5])
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_pack_writes_the_host_bytes_and_unpacks_to_the_text(ctx, name, in_off, out_off):
    import harc_amd
    text, B = CASES[name]
    header = out_off == 0 or len(text) % 2 == 0                   # with and without the file header over the cases
    blob = _pack(ctx, text, B, in_off=in_off, out_off=out_off, header=header)
    want = _host(name)
    assert blob == (want if header else want[32:])
    if not header:
        blob = want[:32] + blob
    assert _unpack(ctx, blob, in_off=in_off, out_off=out_off) == text
    assert harc_amd.sunpack_host(blob) == text


def test_device_pack_size_only_and_capacity_one_byte_short(ctx):
    import harc_amd
    import torch
    name = "markov_3B5_B12000"
    text, B = CASES[name]
    tt, pt = _dev(text, 3)
    torch.cuda.synchronize()
    size = ctx.spack_device(pt, len(text), B)                      # no output: the size alone
    assert size == len(_host(name))
    out = torch.zeros(size + 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(harc_amd.HarcAmdError) as e:
        ctx.spack_device(pt, len(text), B, out.data_ptr(), size - 1)
    assert e.value.code == EINVAL and str(size) in str(e.value) and str(size - 1) in str(e.value), str(e.value)
    assert ctx.spack_device(pt, len(text), B, out.data_ptr(), size) == size
    assert out[:size].cpu().numpy().tobytes() == _host(name)
    # ... and of the unpacked text
    tb, pb = _dev(_host(name), 1)
    torch.cuda.synchronize()
    with pytest.raises(harc_amd.HarcAmdError) as e:
        ctx.sunpack_device(pb, size, out.data_ptr(), len(text) - 1)
    assert e.value.code == EINVAL and str(len(text)) in str(e.value) and str(len(text) - 1) in str(e.value), str(e.value)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_device_unpack_refuses_damaged_blocks_with_the_host_twins_words_and_the_context_goes_on(ctx, mode):
    """eight of the single-bit flips that the sanitizer build of the host test handled cleanly, and for the coded modes a damaged row and a damaged strand size"""
    import harc_amd
    import torch
    text = sc.corruption_texts()[mode]
    packed = harc_amd.spack_host(text)
    assert [m for _, m, _ in sc.blocks_of(packed)] == [mode]
    bad = dict(list(sorted(sc.flips(packed).items()))[:8])
    if mode:
        b = bytearray(packed); b[45 + 32 + (32 if mode == 2 else 0)] ^= 1; bad["frequency"] = bytes(b)       # the first frequency of the first row
        hdr = 45 + 32 + 2 * bin(int.from_bytes(packed[45:77], "little")).count("1") if mode == 1 else None
        if hdr:
            b = bytearray(packed); b[hdr] ^= 1; bad["strand_size"] = bytes(b)
    out = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda")
    for k, blob in sorted(bad.items()):
        with pytest.raises(harc_amd.HarcAmdError) as eh:
            harc_amd.sunpack_host(blob)
        tb, pb = _dev(blob, 5)
        torch.cuda.synchronize()
        with pytest.raises(harc_amd.HarcAmdError) as e:
            ctx.sunpack_device(pb, len(blob), out.data_ptr(), len(text))
        assert e.value.code == EINVAL and "block 0" in str(e.value) and "byte 32" in str(e.value), (k, str(e.value))
        # the same code: the words behind the block's number are the host twin's
        assert str(e.value).split("block 0", 1)[1] == str(eh.value).split("block 0", 1)[1], (k, str(e.value), str(eh.value))
    assert _unpack(ctx, packed) == text                            # the call after them on the same context


# ------------------------------------------------------------------------------------------------ the file calls
def test_file_calls_are_a_function_of_the_text_and_the_block_size_alone(tmp_path, monkeypatch, capfd):
    import harc_amd
    text = sc.cycle(20000) + sc.uniform(20000, seed=2) + sc.skewed(20000, seed=4) + sc.markov(25000, seed=8)
    src = tmp_path / "x.tar"
    src.write_bytes(text)
    want = harc_amd.spack_host(text, 20000)
    assert [m for _, m, _ in sc.blocks_of(want)] == [2, 0, 1, 2, 2]
    monkeypatch.setenv("HARC_AMD_SPACK_BLOCK", "20000")
    for piece, slice_ in (("1", "300"), ("2", "700"), (None, None)):                   # (None: the defaults)
        for k, v in (("HARC_AMD_SPACK_PIECE", piece), ("HARC_AMD_FEED_SLICE", slice_)):
            monkeypatch.setenv(k, v) if v else monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("HARC_AMD_TRACE", "1")
        out = tmp_path / ("x.%s.hs" % piece)
        harc_amd.spack_files(str(src), str(out))
        line = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[spack]")]
        monkeypatch.delenv("HARC_AMD_TRACE")
        assert out.read_bytes() == want, piece
        pieces = (5 + int(piece) - 1) // int(piece) if piece else 1
        assert len(line) == 1 and "%d bytes of text -> %d bytes in 5 blocks (1 stored, 1 order 0, 3 order 1), %d pieces" % (len(text), len(want), pieces) in line[0], line
        back = tmp_path / ("x.%s.back" % piece)
        harc_amd.sunpack_files(str(out), str(back))
        assert back.read_bytes() == text, piece
    # several files on one context
    pairs = [(str(src), str(tmp_path / "l0.hs")), (str(tmp_path / "x.1.back"), str(tmp_path / "l1.hs"))]
    harc_amd.spack_file_list(pairs)
    assert all(open(b, "rb").read() == want for _, b in pairs)
    harc_amd.sunpack_file_list([(b, b + ".back") for _, b in pairs])
    assert all(open(b + ".back", "rb").read() == text for _, b in pairs)
    # a damaged block of a later piece is named by its number and its byte in the file; refusals leave no output
    bad = bytearray(want)
    off = [at for at, _, _ in sc.blocks_of(want)]
    bad[off[3] + 4] = 3
    (tmp_path / "bad.hs").write_bytes(bytes(bad))
    back = tmp_path / "bad.back"
    monkeypatch.setenv("HARC_AMD_SPACK_PIECE", "1")
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.sunpack_files(str(tmp_path / "bad.hs"), str(back))
    with pytest.raises(harc_amd.HarcAmdError) as eh:
        harc_amd.sunpack_host(bytes(bad))
    for err in (e.value, eh.value):
        assert err.code == EINVAL and "block 3 " in str(err) and "byte %d " % off[3] in str(err) and "is damaged" in str(err), str(err)
    assert not back.exists()
    (tmp_path / "cut.hs").write_bytes(want[:-9])
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.sunpack_files(str(tmp_path / "cut.hs"), str(back))
    assert e.value.code == EINVAL and not back.exists()
    with pytest.raises(harc_amd.HarcAmdError):
        harc_amd.spack_files(str(tmp_path / "missing"), str(tmp_path / "missing.hs"))
    assert not (tmp_path / "missing.hs").exists()
    monkeypatch.delenv("HARC_AMD_SPACK_BLOCK")
    (tmp_path / "e").write_bytes(b"")
    harc_amd.spack_files(str(tmp_path / "e"), str(tmp_path / "e.hs"))
    assert (tmp_path / "e.hs").read_bytes() == harc_amd.spack_host(b"")
    harc_amd.sunpack_files(str(tmp_path / "e.hs"), str(tmp_path / "e.back"))
    assert (tmp_path / "e.back").read_bytes() == b""


# ------------------------------------------------------------------------------------------------ ./harc
def _harc(args, env, seconds):
    """every GPU step under its own time limit"""
    return subprocess.run(["timeout", "-k", "10", str(seconds), os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


@pytest.mark.parametrize("flags", [["-p"], []])
def test_harc_packs_the_streams_and_restores_the_reads(tmp_path, flags):
    L, n = 100, 3000
    reads = gen.reads_text(41, n, L, 20000, err=0.01, n_frac=0.25).split()
    assert any(b"N" in r for r in reads)
    got = {}
    for how in ("S", "none"):
        d = tmp_path / how
        d.mkdir()
        fq = d / "x.fastq"
        fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * L) for i, r in enumerate(reads)))
        env = dict(os.environ)
        env.pop("HARC_AMD_STAGE3", None)
        if how == "none":
            env["HARC_AMD_STAGE3"] = "none"
        r = _harc(["-c", str(fq)] + flags + ["-t", "2"] + (["-S"] if how == "S" else []), env, 120)
        assert r.returncode == 0, r.stdout[-2000:]
        assert not (d / "output").exists()
        with tarfile.open(d / "x.harc") as tf:
            names = sorted(os.path.basename(m) for m in tf.getnames() if os.path.basename(m) not in ("", "."))
        streams = ["read_seq.tar", "read_pos.tar", "read_noise.tar", "read_noisepos.tar", "read_rev.tar", "input_N.dna", "read_singleton.txt"]
        streams += ["read_order.bin", "read_order_N.bin", "read_order_N_pe.bin"] if flags else []
        for s in streams:
            assert (s + ".hs" in names) == (how == "S") and (s in names) == (how != "S"), (how, names)
        r = _harc(["-d", str(d / "x.harc")] + flags, env, 120)
        assert r.returncode == 0, r.stdout[-2000:]
        assert not (d / "output").exists()
        got[how] = (d / "x.dna.d").read_bytes()
    assert got["S"] == got["none"]
    if flags:
        assert got["S"] == b"".join(r + b"\n" for r in reads)
    else:
        assert sorted(got["S"].split()) == sorted(reads)
