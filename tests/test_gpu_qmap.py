"""Lossy quality values on the GPU: harc_amd_qmap_device against the serial mapper on the host (the same bytes and statistics whatever the alignment, in place and
out of place, nothing written outside the output), its refusals, the two file calls in small pieces, and ./harc -c -q -b end to end."""
import os
import subprocess

import pytest

from tests import gen
from tests import qmap_cases as mc
from tests import quality_cases as qc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
CASES = mc.cases()
IN_OFFS, OUT_OFFS = (0, 1, 3, 15), (0, 5, 8)
GUARD = 48


@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        yield h


def _placed(b, off):
    """b at `off` bytes behind a 16-byte boundary, 0xEE either side -> (tensor, device address)"""
    import torch
    t = torch.full((off + len(b) + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    if b:
        t[off:off + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + off


def _read(t, off, n):
    """-> the n bytes at off; the guard bytes either side must still be 0xEE"""
    host = t.cpu().numpy().tobytes()
    assert host[:off] == b"\xee" * off and host[off + n:] == b"\xee" * (len(host) - off - n), "bytes outside the text were written"
    return host[off:off + n]


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_mapper_writes_the_host_bytes_at_every_alignment_in_place_and_out_of_place(ctx, name):
    import harc_amd
    import torch
    text, L = CASES[name]
    n = len(text) // (L + 1)
    ins = {off: _placed(text, off) for off in IN_OFFS}
    outs = {off: torch.empty(16 + off + len(text) + GUARD, dtype=torch.uint8, device="cuda") for off in OUT_OFFS}
    for spec in mc.SCHEMES:
        want, wstats = harc_amd.qmap_host(text, L, spec)
        for io in IN_OFFS:
            for oo in OUT_OFFS:
                out = outs[oo].fill_(0xEE)
                torch.cuda.synchronize()                          # the library works on a stream of its own
                stats = ctx.qmap_device(ins[io][1], n, L, spec, out.data_ptr() + 16 + oo)
                assert _read(out, 16 + oo, len(text)) == want and stats == wstats, (spec, io, oo)
            t = ins[io][0].clone()                                 # in place
            torch.cuda.synchronize()
            p = t.data_ptr() + io
            stats = ctx.qmap_device(p, n, L, spec, p)
            assert _read(t, io, len(text)) == want and stats == wstats, (spec, io, "in place")
        out = outs[5].fill_(0xEE)                                  # without the statistics: the same bytes
        torch.cuda.synchronize()
        assert ctx.qmap_device(ins[3][1], n, L, spec, out.data_ptr() + 21, stats=False) is None
        assert _read(out, 21, len(text)) == want, spec
    for io in IN_OFFS:                                             # no out-of-place run changed its input
        assert _read(ins[io][0], io, len(text)) == text


def test_partial_overlap_an_invalid_table_and_a_broken_stride_are_refused_and_the_context_goes_on(ctx):
    import harc_amd
    import torch
    text, L = CASES["L100_300"]
    n = len(text) // (L + 1)
    t, p = _placed(text + b"\xee" * len(text), 3)
    torch.cuda.synchronize()
    for d in (1, 16, len(text) - 1, -1, -3):
        with pytest.raises(harc_amd.HarcAmdError) as e:
            ctx.qmap_device(p, n, L, "ill8", p + d)
        assert e.value.code == EINVAL and "overlap" in str(e.value), str(e.value)
    assert _read(t, 3, 2 * len(text)) == text + b"\xee" * len(text)
    m = harc_amd.qmap_parse("ill8")
    m.table[10] = 32
    with pytest.raises(harc_amd.HarcAmdError) as e:
        ctx.qmap_device(p, n, L, m, p)
    assert e.value.code == EINVAL and "byte value 10 " in str(e.value), str(e.value)
    m = harc_amd.qmap_parse("pblock:2")
    m.radius = 47
    with pytest.raises(harc_amd.HarcAmdError) as e:
        ctx.qmap_device(p, n, L, m, p)
    assert e.value.code == EINVAL and "radius 47" in str(e.value), str(e.value)
    for at, byte, counts in ((150 * 101 + 40, 10, "0 positions on the 101-byte stride hold no newline and 1 newlines"),
                             (150 * 101 + 100, ord("I"), "1 positions on the 101-byte stride hold no newline and 0 newlines")):
        b = bytearray(text)
        b[at] = byte
        tb, pb = _placed(bytes(b), 5)
        out = torch.zeros(len(b) + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for spec in ("cap:30", "pblock:2"):
            with pytest.raises(harc_amd.HarcAmdError) as e:
                ctx.qmap_device(pb, n, L, spec, out.data_ptr())
            with pytest.raises(harc_amd.HarcAmdError) as eh:
                harc_amd.qmap_host(bytes(b), L, spec)
            assert e.value.code == EINVAL and counts in str(e.value) and str(e.value) == str(eh.value), str(e.value)
    want, wstats = harc_amd.qmap_host(text, L, "pblock:4")         # the call after them on the same context
    assert ctx.qmap_device(p, n, L, "pblock:4", p) == wstats and _read(t, 3, 2 * len(text)) == want + b"\xee" * len(text)


# ------------------------------------------------------------------------------------------------ the file calls
@pytest.mark.parametrize("n,L", [(901, 50), (300, 255)])
def test_qmap_files_is_the_host_mappers_file_whatever_the_pieces(tmp_path, monkeypatch, n, L):
    import harc_amd
    text = qc.markov(n, L, seed=n)
    q = tmp_path / "x.quality"
    q.write_bytes(text)
    monkeypatch.setenv("HARC_AMD_FEED_SLICE", str(3 * (L + 1) + 7))
    for spec in ("ill8", "pblock:2"):
        want, wstats = harc_amd.qmap_host(text, L, spec)
        for piece, threads in (("7", "2"), ("256", "16"), (None, "1")):
            if piece:
                monkeypatch.setenv("HARC_AMD_QMAP_PIECE", piece)
            else:
                monkeypatch.delenv("HARC_AMD_QMAP_PIECE")
            monkeypatch.setenv("HARC_AMD_FEED_THREADS", threads)
            out = tmp_path / ("x.%s.%s" % (spec.replace(":", "_"), piece))
            assert harc_amd.qmap_files(str(q), str(out), spec) == wstats, (spec, piece)
            assert out.read_bytes() == want, (spec, piece)
    assert q.read_bytes() == text
    # refusals: the input as the output (kept), and a file that is no whole lines (no output left)
    monkeypatch.setenv("HARC_AMD_QMAP_PIECE", "7")
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.qmap_files(str(q), str(q), "ill8")
    assert e.value.code == EINVAL and q.read_bytes() == text
    (tmp_path / "cut.quality").write_bytes(text[:-3])
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.qmap_files(str(tmp_path / "cut.quality"), str(tmp_path / "cut.out"), "ill8")
    assert e.value.code == EINVAL and not (tmp_path / "cut.out").exists()
    bad = bytearray(text)
    bad[(n - 2) * (L + 1) + L] = ord("I")                          # a stride position of the last piece
    (tmp_path / "bad.quality").write_bytes(bytes(bad))
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.qmap_files(str(tmp_path / "bad.quality"), str(tmp_path / "bad.out"), "pblock:2")
    assert e.value.code == EINVAL and "stride" in str(e.value) and not (tmp_path / "bad.out").exists()
    (tmp_path / "e.quality").write_bytes(b"")
    assert harc_amd.qmap_files(str(tmp_path / "e.quality"), str(tmp_path / "e.out"), "ill8")["values"] == 0 and (tmp_path / "e.out").read_bytes() == b""


def test_qpack_files_with_a_spec_is_qpack_files_of_the_mapped_file(tmp_path, monkeypatch, capfd):
    import harc_amd
    L, n = 100, 5000
    text = qc.markov(n, L, seed=23)
    q = tmp_path / "x.quality"
    q.write_bytes(text)
    monkeypatch.setenv("HARC_AMD_QPACK_BLOCK", "300")
    monkeypatch.setenv("HARC_AMD_QPACK_PIECE", "1")
    monkeypatch.setenv("HARC_AMD_FEED_SLICE", "256")
    monkeypatch.setenv("HARC_AMD_TRACE", "1")
    for spec in ("ill8", "pblock:2"):
        mapped, wstats = harc_amd.qmap_host(text, L, spec)
        mq = tmp_path / "mapped.quality"
        mq.write_bytes(mapped)
        assert harc_amd.qpack_files(str(mq), str(tmp_path / "want.hq")) is None
        plain = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[qpack]")]
        assert harc_amd.qpack_files(str(q), str(tmp_path / "got.hq"), spec=spec) == wstats
        lossy = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[qpack]")]
        assert (tmp_path / "got.hq").read_bytes() == (tmp_path / "want.hq").read_bytes() == harc_amd.qpack_host(mapped, L, 300)
        assert len(plain) == 1 and "map" not in plain[0] and len(lossy) == 1 and "in the kernels of the map" in lossy[0], (plain, lossy)
        harc_amd.qunpack_files(str(tmp_path / "got.hq"), str(tmp_path / "back.quality"))
        assert (tmp_path / "back.quality").read_bytes() == mapped
        capfd.readouterr()                                         # (the unpacker's own [qpack] line)
    assert q.read_bytes() == text                                  # the mapped text never reached a file
    m = harc_amd.qmap_parse("ill8")
    m.table[0] = 1
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.qpack_files(str(q), str(tmp_path / "bad.hq"), spec=m)
    assert e.value.code == EINVAL and "byte value 0 " in str(e.value) and not (tmp_path / "bad.hq").exists()


# ------------------------------------------------------------------------------------------------ ./harc
def _harc(args, env):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


@pytest.mark.parametrize("spec,pack", [("ill8", True), ("pblock:2", False)])
def test_harc_maps_the_quality_values_and_restores_everything_else(tmp_path, spec, pack):
    """-p on both sides: x.d.fastq is the input with its quality lines mapped by the Python twin, ids and reads as they were"""
    L, n = 100, 3000
    reads = gen.reads_text(33, n, L, 20000, err=0.01, n_frac=0.25).split()
    assert any(b"N" in r for r in reads)
    qtext = qc.markov(len(reads), L, seed=19)
    quals = qtext.split()
    ids = [b"@run9.%d len=%d/%d" % (i, L, 1 + i % 2) for i in range(len(reads))]
    fq = tmp_path / "x.fastq"
    fq.write_bytes(b"".join(b"%s\n%s\n+\n%s\n" % t for t in zip(ids, reads, quals)))
    env = dict(os.environ, HARC_AMD_STAGE3="none")
    r = _harc(["-c", str(fq), "-q", "-p"] + (["-Q"] if pack else []) + ["-b", spec, "-t", "2"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("[qmap] %s: %d values, " % (spec, len(reads) * L))]
    assert len(line) == 1, r.stdout[-2000:]
    mapped, stats = mc.mapped(qtext, L, spec)
    assert "%d changed" % stats["changed"] in line[0] and "max change %d" % stats["max_abs"] in line[0], line
    assert "distinct values %d -> %d" % (stats["distinct_in"], stats["distinct_out"]) in line[0], line
    assert (tmp_path / "x.quality.hq").exists() == pack and (tmp_path / "x.quality").exists() != pack
    assert not (tmp_path / "x.quality.tmp").exists() and not (tmp_path / "output").exists()
    if not pack:
        assert (tmp_path / "x.quality").read_bytes() == mapped
    r = _harc(["-d", str(tmp_path / "x.harc"), "-q", "-p"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert (tmp_path / "x.d.fastq").read_bytes() == b"".join(b"%s\n%s\n+\n%s\n" % t for t in zip(ids, reads, mapped.split()))
