"""Plain gzip input inflated on the GPU: harc_amd_gunzip_device against Python's gzip and against harc_amd_gunzip_host (text, statistics, guard bytes) on every case
of tests/gunzip_cases.py, harc_amd_gunzip_files in pieces that cut blocks and carry the window, damaged input refused with EINVAL and no output file, and ./harc
end to end.  The shapes are the smallest at which the kernels can go wrong; the host build of the same decoder is fuzzed under sanitizers in
tests/test_gunzip_host.py."""
import gzip
import os
import re
import subprocess
import tarfile

import pytest

from tests import bgzf_util as bu
from tests import gunzip_cases as gc

pytestmark = pytest.mark.gpu
ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5


@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        yield h


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda") if b else torch.empty(16, dtype=torch.uint8, device="cuda")


def _gunzip(h, blob, chunk_bytes, shift=0):
    """-> (text, stats); the output sits `shift` bytes off a 256-byte boundary between two guard zones, which must come back untouched"""
    import torch
    d = _dev(blob)
    n, _ = h.gunzip_device(d.data_ptr(), len(blob), chunk_bytes=chunk_bytes)
    lo = 256 + shift
    buf = torch.full((lo + n + 256,), GUARD, dtype=torch.uint8, device="cuda")
    got, st = h.gunzip_device(d.data_ptr(), len(blob), buf.data_ptr() + lo, n, chunk_bytes=chunk_bytes)
    torch.cuda.synchronize()
    assert got == n
    host = buf.cpu().numpy().tobytes()
    assert host[:lo] == bytes([GUARD]) * lo and host[lo + n:] == bytes([GUARD]) * 256, "a byte outside the text was written"
    return host[lo:lo + n], st


@pytest.mark.parametrize("name", sorted(gc.valid_cases()))
def test_device_equals_gzip_and_the_host_restatement(ctx, name):
    import harc_amd
    blob, text = gc.valid_cases()[name]
    for i, cb in enumerate(gc.CHUNKS):
        got, st = _gunzip(ctx, blob, cb, shift=(0, 3, 16)[i])
        assert got == text, (name, cb)
        assert st == harc_amd.gunzip_host(blob, cb)[1], (name, cb)


def test_device_small_texts_and_a_buffer_that_is_too_small(ctx):
    import harc_amd
    base = bu.fastq_text(200, 100, seed=8)
    for n in (0, 1, 15, 16, 17, 63, 64, 65, 16383, 16384, 16385):
        assert _gunzip(ctx, gzip.compress(base[:n], 6), 0, shift=n % 5)[0] == base[:n]
    blob, text = gc.valid_cases()["e_header_fields"]
    d = _dev(blob)
    with pytest.raises(harc_amd.HarcAmdError) as e:
        ctx.gunzip_device(d.data_ptr(), len(blob), d.data_ptr(), len(text) - 1)
    assert e.value.code == -1 and str(len(text)) in str(e.value)


@pytest.mark.parametrize("name", ["a_level6", "c_far_matches"])
@pytest.mark.parametrize("geom", ["pieces", "pieces_chunks_budget", "default"])
def test_files_in_pieces_that_cut_blocks(name, geom, tmp_path, monkeypatch):
    """pieces of 48 KiB of compressed bytes through slices of 6000 bytes: blocks of 19-20 KB straddle every piece cut, and what lies behind the last block
    boundary of a piece is carried into the next with the bit offset and the window"""
    import harc_amd
    blob, text = gc.valid_cases()[name]
    if geom != "default":
        monkeypatch.setenv("HARC_AMD_GUNZIP_PIECE", str(48 << 10))
        monkeypatch.setenv("HARC_AMD_FEED_SLICE", "6000")
    if geom == "pieces_chunks_budget":                               # several chunks a piece, and a piece's text in several turns
        monkeypatch.setenv("HARC_AMD_GUNZIP_CHUNK", "8192")
        monkeypatch.setenv("HARC_AMD_GUNZIP_BUDGET", "60000")
    gz, out = tmp_path / "x.gz", tmp_path / "x.txt"
    gz.write_bytes(blob)
    st = harc_amd.gunzip_files(str(gz), str(out))
    assert out.read_bytes() == text
    assert st["members"] == 1 and st["text_bytes"] == len(text)
    if geom != "default":
        assert st["chunks"] >= len(blob) // (48 << 10)              # at least one chunk a piece


def test_files_with_several_members(tmp_path, monkeypatch):
    import harc_amd
    blob, text = gc.valid_cases()["d_three_members"]
    gz, out = tmp_path / "x.gz", tmp_path / "x.txt"
    gz.write_bytes(blob)
    for piece in (None, 20000):
        if piece:
            monkeypatch.setenv("HARC_AMD_GUNZIP_PIECE", str(piece))
            monkeypatch.setenv("HARC_AMD_FEED_SLICE", "4096")
        st = harc_amd.gunzip_files(str(gz), str(out))
        assert out.read_bytes() == text and st["members"] == 3


@pytest.mark.parametrize("name", sorted(gc.damaged_cases()))
def test_damage_is_refused_and_leaves_no_file(ctx, name, tmp_path, monkeypatch):
    """refusals by a decoder that validates before it trusts: nothing here is meant to fault"""
    import harc_amd
    blob = gc.damaged_cases()[name]
    d = _dev(blob)
    for cb in (32 << 10, 0):
        with pytest.raises(harc_amd.HarcAmdError) as e:
            import torch
            out = torch.empty(len(gc.text_a()) + 64, dtype=torch.uint8, device="cuda")
            ctx.gunzip_device(d.data_ptr(), len(blob), out.data_ptr(), len(gc.text_a()) + 48, chunk_bytes=cb)
        assert e.value.code == -1 and re.search(r"compressed byte \d+", str(e.value)), str(e.value)
    gz, out = tmp_path / "bad.gz", tmp_path / "bad.txt"
    gz.write_bytes(blob)
    for piece in (None, 48 << 10):
        if piece:
            monkeypatch.setenv("HARC_AMD_GUNZIP_PIECE", str(piece))
        with pytest.raises(harc_amd.HarcAmdError) as e:
            harc_amd.gunzip_files(str(gz), str(out))
        assert e.value.code == -1 and re.search(r"compressed byte \d+", str(e.value)), str(e.value)
        assert not out.exists()
    good, text = gc.valid_cases()["e_header_fields"]
    assert _gunzip(ctx, good, 0)[0] == text                         # the context still works


def _harc(args, env=None):
    return subprocess.run([os.path.join(ROOT_DIR, "harc")] + args, cwd=ROOT_DIR, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)


def _members(arc):
    """{member: bytes}; a stream tar inside the archive as {file: bytes} (a tar header holds the time of the run)"""
    import io
    with tarfile.open(arc) as tf:
        out = {os.path.basename(m.name): tf.extractfile(m).read() for m in tf.getmembers() if m.isfile()}
    for n in [n for n in out if n.endswith(".tar")]:
        with tarfile.open(fileobj=io.BytesIO(out[n])) as tf:
            out[n] = {os.path.basename(m.name): tf.extractfile(m).read() for m in tf.getmembers() if m.isfile()}
    return out


def test_harc_cli_on_plain_gzip_end_to_end(tmp_path):
    """HARC_AMD_GUNZIP=1 ./harc -c x.fastq.gz -p -q on gzip's own output: inflated by the stage program, the archive and the side files are those of the plain file, and
    ./harc -d -p -q gives the FASTQ back"""
    text = bu.fastq_text(2000, 100, seed=31)
    env = dict(os.environ, HARC_AMD_STAGE3="none", HARC_AMD_GUNZIP="1")
    got = {}
    for kind in ("plain", "gzip"):
        d = tmp_path / kind
        d.mkdir()
        f = d / ("x.fastq" if kind == "plain" else "x.fastq.gz")
        f.write_bytes(text if kind == "plain" else gzip.compress(text, 6))
        r = _harc(["-c", str(f), "-p", "-q"], env)
        assert r.returncode == 0, r.stdout[-2000:]
        assert ("[gunzip] 1 members" in r.stdout) == (kind == "gzip") and "on the host" not in r.stdout, r.stdout[-2000:]
        assert (d / "x.harc").exists() and not (d / "output").exists()
        got[kind] = (_members(d / "x.harc"), (d / "x.quality").read_bytes(), (d / "x.id").read_bytes())
    assert sorted(got["plain"][0]) == sorted(got["gzip"][0]) and ".input.fastq" not in got["gzip"][0]
    differ = [n for n in got["plain"][0] if got["plain"][0][n] != got["gzip"][0][n]]
    assert not differ, differ
    assert got["plain"][1:] == got["gzip"][1:]
    r = _harc(["-d", str(tmp_path / "gzip" / "x.harc"), "-p", "-q"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert (tmp_path / "gzip" / "x.d.fastq").read_bytes() == text


def test_harc_cli_on_plain_gzip_with_two_ranks_on_one_device(tmp_path):
    text = bu.fastq_text(2000, 100, seed=32)
    f = tmp_path / "x.fastq.gz"
    f.write_bytes(gzip.compress(text, 6))
    env = dict(os.environ, HARC_AMD_XPORT="mailbox", HARC_AMD_SHARE_DEVICE="0", HARC_AMD_MAILBOX_TIMEOUT="120", HARC_AMD_STAGE3="none", HARC_AMD_GUNZIP="1")
    r = _harc(["-c", str(f), "-p", "-q", "-g", "2"], env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "[gunzip] 1 members" in r.stdout and "on the host" not in r.stdout, r.stdout[-2000:]
    r = _harc(["-d", str(tmp_path / "x.harc"), "-p", "-q"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert (tmp_path / "x.d.fastq").read_bytes() == text
