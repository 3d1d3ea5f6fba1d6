"""The GPU inflate on DEFLATE streams that zlib's encoder never writes (tests/foreign_deflate_cases.py): harc_amd_gunzip_device against zlib and against
harc_amd_gunzip_host (text, statistics, guard bytes) at chunks of 64 and 1000 bytes and the default, with the text cut into turns that carry the window, as files
in pieces that carry it, the refusals of what zlib refuses, and the same streams as BGZF members.  What only the device runs is what these reach: k_gz_translate's
search for the walk of a text byte where walks are empty, k_gz_window over many short walks, k_gz_find's stride over more than 1024 chunks, and indices 0 to 261
of the window in front of a walk, which a distance above 32 506 alone reads.  The host build of the same decoder runs them under sanitizers in
tests/test_gunzip_host.py and tests/test_bgzf_host.py."""
import re

import pytest

from tests import bgzf_util as bu
from tests import foreign_deflate_cases as fc

pytestmark = pytest.mark.gpu
GUARD = 0xA5
CHUNKS = (64, 1000, 0)
BUDGETS = ((1000, 41000), (1000, 35000), (64, None))               # (chunk bytes, budget; None: the D + 3000 literals): tests/test_gunzip_host.py says what each cuts


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


@pytest.mark.parametrize("name", sorted(fc.valid_cases()))
def test_device_equals_zlib_and_the_host_restatement(ctx, name):
    import harc_amd
    blob, text = fc.valid_cases()[name]
    for i, cb in enumerate(CHUNKS):
        got, st = _gunzip(ctx, blob, cb, shift=(0, 3, 16)[i])
        assert got == text, (name, cb)
        assert st == harc_amd.gunzip_host(blob, cb)[1], (name, cb)


@pytest.mark.parametrize("D", fc.FAR)
def test_device_budget_turns_carry_the_window(ctx, D, monkeypatch):
    import harc_amd
    blob, text = fc.valid_cases()[f"far_{D}"]
    for i, (cb, budget) in enumerate(BUDGETS):
        monkeypatch.setenv("HARC_AMD_GUNZIP_BUDGET", str(budget or D + 3000))
        got, st = _gunzip(ctx, blob, cb, shift=(0, 3, 16)[i])
        assert got == text, (D, cb, budget)
        assert st == harc_amd.gunzip_host(blob, cb)[1], (D, cb, budget)


@pytest.mark.parametrize("name", ["far_32768", "far_32507", "stored_65535", "empty_walks"])
@pytest.mark.parametrize("geom", ["pieces", "default"])
def test_files_in_pieces_that_carry_the_window(name, geom, tmp_path, monkeypatch):
    """pieces of 8192 compressed bytes through slices of 4096, chunks of 1000: a match at distance 32 768 behind a piece cut reads the window that the state
    carries, and a stored block of 65 535 bytes is carried until all of it is there"""
    import harc_amd
    blob, text = fc.valid_cases()[name]
    if geom == "pieces":
        monkeypatch.setenv("HARC_AMD_GUNZIP_PIECE", "8192")
        monkeypatch.setenv("HARC_AMD_FEED_SLICE", "4096")
        monkeypatch.setenv("HARC_AMD_GUNZIP_CHUNK", "1000")
    gz, out = tmp_path / "x.gz", tmp_path / "x.txt"
    gz.write_bytes(blob)
    st = harc_amd.gunzip_files(str(gz), str(out))
    assert out.read_bytes() == text
    assert st["members"] == 1 and st["text_bytes"] == len(text)


@pytest.mark.parametrize("name", sorted(fc.refused_cases()))
def test_what_zlib_refuses_is_refused_and_leaves_no_file(ctx, name, tmp_path):
    """refusals by a decoder that validates before it trusts: nothing here is meant to fault.  Each of these streams is refused by the host build of the same
    decoder under sanitizers and by harc_amd_gunzip_host (tests/test_gunzip_host.py)"""
    import harc_amd
    import torch
    blob = fc.refused_cases()[name][0]
    d = _dev(blob)
    out = torch.empty(65536 + 64, dtype=torch.uint8, device="cuda")
    for cb in (1000, 0):
        with pytest.raises(harc_amd.HarcAmdError) as e:
            ctx.gunzip_device(d.data_ptr(), len(blob), out.data_ptr(), 65536, chunk_bytes=cb)
        m = re.search(r"compressed byte (\d+)", str(e.value))
        assert e.value.code == -1 and m and int(m.group(1)) <= len(blob), str(e.value)
        with pytest.raises(harc_amd.HarcAmdError) as h:
            harc_amd.gunzip_host(blob, cb)
        assert str(h.value) == str(e.value)                         # the host restatement names the same byte for the same reason
    gz, txt = tmp_path / "bad.gz", tmp_path / "bad.txt"
    gz.write_bytes(blob)
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.gunzip_files(str(gz), str(txt))
    assert e.value.code == -1 and re.search(r"compressed byte \d+", str(e.value)), str(e.value)
    assert not txt.exists()
    good, text = fc.valid_cases()["one_dist_and_empties"]
    assert _gunzip(ctx, good, 0)[0] == text                         # the context still works


def _inflate(h, blob):
    import torch
    d = _dev(blob)
    n = h.bgzf_inflate_device(d.data_ptr(), len(blob))
    out = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    assert h.bgzf_inflate_device(d.data_ptr(), len(blob), out.data_ptr(), n) == n
    torch.cuda.synchronize()
    return out[:n].cpu().numpy().tobytes()


def test_bgzf_crafted_members_among_zlibs(ctx):
    """a BGZF file whose members are zlib's and crafted ones in turn gives the text; with one refused member in it, it is refused naming that member"""
    import harc_amd
    fq = bu.fastq_text(300, 100, seed=17)
    parts, texts = [], []
    for i, (m, text) in enumerate(fc.bgzf_members().values()):
        piece = fq[i * 2000:(i + 1) * 2000]
        parts += [bu.bgzf(piece, 999, 6, eof=False), m]
        texts += [piece, text]
    good = b"".join(parts) + bu.EOF_MARKER
    assert _inflate(ctx, good) == b"".join(texts)
    for name, bad in fc.bgzf_refused_members().items():
        at = len(b"".join(parts[:5]))
        blob = b"".join(parts[:5]) + bad + b"".join(parts[5:]) + bu.EOF_MARKER
        with pytest.raises(harc_amd.HarcAmdError) as e:
            _inflate(ctx, blob)
        assert e.value.code == -1 and str(at) in str(e.value), (name, str(e.value))
    assert _inflate(ctx, good) == b"".join(texts)                   # the context still works
