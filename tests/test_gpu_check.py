"""Checked archives on the GPU: harc_amd_text_digest_device against the numpy model at every size, alignment and offset at which the kernel takes another path, the
file call in small pieces, the order digest of an ingested FASTQ, and ./harc -c -V / -d / -v end to end: what read.check records, what -d and -v check, and what
they refuse -- a changed stream byte (which an archive made without -V decodes without a word), reads in another order, a changed side file."""
import functools
import io
import os
import shutil
import subprocess
import tarfile

import pytest

from tests import bgzf_util
from tests import check_cases as cc
from tests import gen
from tests import id_cases
from tests import qmap_cases as mc
from tests import quality_cases as qc
from tests.bucket_ref import reads_signature

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65537, (1 << 20) + 3)
OFFS = (0, 1, 3, 7)
N_READS = 3000


@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        yield h


@functools.lru_cache(maxsize=None)
def _text(n, seed=7):
    """n bytes of a FASTQ-like alphabet, about one newline in twelve bytes"""
    import numpy as np
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGTN\n@:0123", dtype=np.uint8)[rng.integers(0, 12, n)].tobytes()


def _on_device(b, lead):
    """b at `lead` bytes behind the start of an allocation -> (tensor, device address of b)"""
    import torch
    t = torch.full((lead + len(b) + 64,), 0x0A, dtype=torch.uint8, device="cuda")      # newlines around the text: a byte that is counted by mistake shows
    if b:
        t[lead:lead + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()                                          # the library works on a stream of its own
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + lead


# ------------------------------------------------------------------------------------------------ the kernel
def test_the_device_digest_is_the_models_at_every_size_and_alignment(ctx):
    text = _text(SIZES[-1])
    placed = {off: _on_device(text, off) for off in OFFS}
    for n in SIZES:
        want = cc.text_digest(text[:n])
        for off in OFFS:
            assert ctx.text_digest_device(placed[off][1], n) == want, (n, off)
    # a text that does not start at the start of its buffer's text: every start inside a 16-byte chunk, a few lengths each
    t, p = placed[0]
    for start in range(1, 17):
        for n in (1, 14, 15, 16, 17, 31, 33, 1000):
            assert ctx.text_digest_device(p + start, n) == cc.text_digest(text[start:start + n]), (start, n)
    assert ctx.text_digest_device(0, 0) == (0, 0, 0)


def test_positions_are_64_bit_numbers(ctx):
    text = _text(100, seed=9)
    t, p = _on_device(text, 5)
    got = {}
    for first in (0, (1 << 32) - 5, (1 << 40) + 1):
        got[first] = ctx.text_digest_device(p, 100, first_offset=first)
        assert got[first] == cc.text_digest(text, first), first
    assert len({g[2] for g in got.values()}) == 3


def test_two_pieces_add_up_to_the_whole(ctx):
    text = _text(70001, seed=11)
    t, p = _on_device(text, 3)
    whole = ctx.text_digest_device(p, len(text))
    assert whole == cc.text_digest(text)
    for cut in (0, 1, 16, 4097, 35000, 70000, 70001):
        a = ctx.text_digest_device(p, cut)
        assert ctx.text_digest_device(p + cut, len(text) - cut, first_offset=cut, acc=a) == whole, cut
        b = ctx.text_digest_device(p + cut, len(text) - cut, first_offset=cut)      # ... in the other order
        assert ctx.text_digest_device(p, cut, acc=b) == whole, cut


def test_the_file_call_gives_the_models_triple_whatever_the_slices_and_threads(tmp_path, monkeypatch):
    import harc_amd
    text = _text(300000, seed=13)
    f = tmp_path / "x.txt"
    f.write_bytes(text)
    want = cc.text_digest(text)
    assert harc_amd.text_digest_file(str(f)) == want
    for sl in ("256", "700"):
        for threads in ("1", "16"):
            monkeypatch.setenv("HARC_AMD_FEED_SLICE", sl)
            monkeypatch.setenv("HARC_AMD_FEED_THREADS", threads)
            assert harc_amd.text_digest_file(str(f)) == want, (sl, threads)
    (tmp_path / "e.txt").write_bytes(b"")
    assert harc_amd.text_digest_file(str(tmp_path / "e.txt")) == (0, 0, 0)
    with pytest.raises(harc_amd.HarcAmdError):
        harc_amd.text_digest_file(str(tmp_path / "none.txt"))
    # the decoders' output read once: both values
    L, n = 33, 1234
    reads = gen.reads_text(5, n, L, 9000, err=0.01, n_frac=0.25).split()
    (tmp_path / "x.dna").write_bytes(b"".join(r + b"\n" for r in reads))
    sig, t = harc_amd.reads_check_file(str(tmp_path / "x.dna"))
    assert sig == reads_signature(reads) and t == cc.text_digest(b"".join(r + b"\n" for r in reads))


# ------------------------------------------------------------------------------------------------ inputs of the CLI tests
@functools.lru_cache(maxsize=None)
def _input(L, swap=False):
    """-> (reads, ids, quality lines) of N_READS records, reads with N among them; swap: records 10 and 2000 exchanged"""
    reads = gen.reads_text(41 + L, N_READS, L, 20000, err=0.01, n_frac=0.25).split()
    if b"N" in reads[-1]:                                          # a clean last read: without -p the id file of an input whose last read has N is a line short (README)
        j = max(i for i, r in enumerate(reads) if b"N" not in r)
        reads[j], reads[-1] = reads[-1], reads[j]
    assert len(reads) == N_READS and any(b"N" in r for r in reads) and reads[10] != reads[2000]
    ids = id_cases.ids(N_READS)
    quals = qc.markov(N_READS, L, seed=17).split()
    rec = list(zip(ids, reads, quals))
    if swap:
        rec[10], rec[2000] = rec[2000], rec[10]
    return tuple(r[1] for r in rec), tuple(r[0] for r in rec), tuple(r[2] for r in rec)


def _fastq(inp):
    reads, ids, quals = inp
    return b"".join(b"%s\n%s\n+\n%s\n" % t for t in zip(ids, reads, quals))


def _lines(ls):
    return b"".join(l + b"\n" for l in ls)


def _harc(args, env):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _env(**kw):
    env = dict(os.environ, HARC_AMD_STAGE3="none")
    env.update(kw)
    return env


def _members(arc):
    with tarfile.open(arc) as t:
        return {m.name[2:]: t.extractfile(m).read() for m in t.getmembers() if m.isfile()}


def _flat(members):
    """the members of an archive with every stream tar replaced by the files in it (a tar holds the time its files were written)"""
    out = {}
    for name, data in members.items():
        if name.endswith(".tar"):
            with tarfile.open(fileobj=io.BytesIO(data)) as t:
                for m in t.getmembers():
                    if m.isfile():
                        out[name + ":" + os.path.basename(m.name)] = t.extractfile(m).read()
        else:
            out[name] = data
    return out


def _record(arc):
    return cc.parse_check(_members(arc)["read.check"])


def _listing(d):
    return sorted((p.name, p.stat().st_size) for p in d.iterdir())


def _check_line(out):
    l = [x for x in out.splitlines() if x.startswith("[check] ")]
    assert len(l) == 1, out[-2000:]
    return l[0]


# ------------------------------------------------------------------------------------------------ ./harc -c -V, -d, -v
FLAGS = (["-V"], ["-p", "-V"], ["-p", "-q", "-V"], ["-q", "-Q", "-I", "-V"], ["-p", "-q", "-Q", "-b", "ill8", "-V"])
CASES = [(L, k, False) for L in (33, 100) for k in range(len(FLAGS))] + [(100, 2, True)]


def _case_env(spack):
    return _env() if not spack else {k: v for k, v in os.environ.items() if k != "HARC_AMD_STAGE3"}      # (-S does not go with a packer of stage III)


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """(L, k, spack) -> the directory in which ./harc -c <FLAGS[k]> [-S] has run on x.fastq, once per case: the -c run is the first of the three tests' that asks"""
    done = {}

    def get(L, k, spack):
        if (L, k, spack) not in done:
            d = tmp_path_factory.mktemp("c%d_%d_%d" % (L, k, spack))
            (d / "x.fastq").write_bytes(_fastq(_input(L)))
            r = _harc(["-c", str(d / "x.fastq"), "-t", "2"] + FLAGS[k] + (["-S"] if spack else []), _case_env(spack))
            assert r.returncode == 0, r.stdout[-2000:]
            done[(L, k, spack)] = d
        return done[(L, k, spack)]
    return get


def _mapped_or_not(quals, L, flags):
    return mc.mapped(_lines(quals), L, "ill8")[0] if "-b" in flags else _lines(quals)


@pytest.mark.parametrize("L,k,spack", CASES)
def test_harc_records_the_models_digests(made, tmp_path, L, k, spack):
    import harc_amd
    flags = FLAGS[k]
    reads, ids, quals = _input(L)
    d = made(L, k, spack)
    members = _members(d / "x.harc")
    assert ("read_seq.tar.hs" in members) == spack and not (d / "output").exists() and not [n for n in members if n.startswith(".check")]
    rec = cc.parse_check(members["read.check"])
    po, pq = "-p" in flags, "-q" in flags
    assert sorted(rec) == sorted(["reads"] + (["order"] if po else []) + (["ids", "quality"] if pq else []))
    assert rec["reads"] == reads_signature(list(reads))
    if po:
        assert rec["order"] == cc.order_digest(reads) and rec["order"][0] == N_READS * (L + 1)
    if pq:
        # the side texts as -c left them; a packed one is unpacked by the library
        qtext, itext = d / "x.quality", d / "x.id"
        assert qtext.exists() != ("-Q" in flags) and itext.exists() != ("-I" in flags) and not (d / "x.quality.tmp").exists()
        if "-Q" in flags:
            harc_amd.qunpack_files(str(d / "x.quality.hq"), str(tmp_path / "back.quality"))
            qtext = tmp_path / "back.quality"
        if "-I" in flags:
            harc_amd.idunpack_files(str(d / "x.id.hi"), str(tmp_path / "back.id"))
            itext = tmp_path / "back.id"
        qbytes, ibytes = qtext.read_bytes(), itext.read_bytes()
        assert rec["quality"] == cc.text_digest(qbytes) and rec["ids"] == cc.text_digest(ibytes)
        want_q = _mapped_or_not(quals, L, flags)
        if po:                                                     # input order: the texts are the input's own (with -b: the Python twin's mapped values)
            assert qbytes == want_q and ibytes == _lines(ids)
            assert rec["quality"] == cc.text_digest(want_q) and rec["ids"] == cc.text_digest(_lines(ids))
        else:
            assert sorted(qbytes.split()) == sorted(want_q.split())


@pytest.mark.parametrize("L,k,spack", CASES)
@pytest.mark.parametrize("mode", ["-v", "-d"])
def test_harc_d_and_v_check_what_is_recorded(made, mode, L, k, spack):
    flags = FLAGS[k]
    reads, ids, quals = _input(L)
    d = made(L, k, spack)
    po, pq = "-p" in flags, "-q" in flags
    want_line = "[check] reads ok, " + ("order ok" if po else "order not checked (no -p)") + (", ids ok, quality ok" if pq else ", ids not checked (no -q), quality not checked (no -q)")
    before = _listing(d)
    r = _harc([mode, str(d / "x.harc")] + (["-p"] if po else []) + (["-q"] if pq else []), _case_env(spack))
    assert r.returncode == 0 and _check_line(r.stdout) == want_line, r.stdout[-2000:]
    assert not (d / "output").exists()
    if mode == "-v":
        assert _listing(d) == before
        return
    out = d / ("x.d.fastq" if pq else "x.dna.d")
    if pq and po:
        assert out.read_bytes() == b"".join(b"%s\n%s\n+\n%s\n" % t for t in zip(ids, reads, _mapped_or_not(quals, L, flags).split()))
    elif po:
        assert out.read_bytes() == _lines(reads)
    elif not pq:
        assert sorted(out.read_bytes().split()) == sorted(reads)
    os.remove(out)


@pytest.mark.parametrize("L", [33, 100])
def test_the_hq_of_the_V_route_is_the_hq_of_the_one_call_that_maps_in_front_of_the_coder(made, tmp_path, L):
    """-b -Q -V maps into a file and packs that without a spec; -b -Q alone maps in device memory in front of the coder: the same X.quality.hq, byte for byte"""
    k = 4
    d = made(L, k, False)
    (tmp_path / "x.fastq").write_bytes(_fastq(_input(L)))
    r = _harc(["-c", str(tmp_path / "x.fastq"), "-t", "2"] + [f for f in FLAGS[k] if f != "-V"], _env())
    assert r.returncode == 0, r.stdout[-2000:]
    assert (tmp_path / "x.quality.hq").read_bytes() == (d / "x.quality.hq").read_bytes()
    assert "read.check" not in _members(tmp_path / "x.harc")


def test_the_record_does_not_depend_on_the_pieces_of_the_ingest_or_on_bgzf(tmp_path):
    L = 100
    inp = _input(L)
    reads = inp[0]
    want = {"reads": reads_signature(list(reads)), "order": cc.order_digest(reads)}
    (tmp_path / "x.fastq").write_bytes(_fastq(inp))
    r = _harc(["-c", str(tmp_path / "x.fastq"), "-p", "-V", "-t", "2"], _env(HARC_AMD_INGEST_CHUNK="50000"))      # a dozen pieces
    assert r.returncode == 0, r.stdout[-2000:]
    assert _record(tmp_path / "x.harc") == want
    r = _harc(["-d", str(tmp_path / "x.harc"), "-p"], _env(HARC_AMD_BIN_READS="500"))
    assert r.returncode == 0 and _check_line(r.stdout) == "[check] reads ok, order ok, ids not checked (no -q), quality not checked (no -q)", r.stdout[-2000:]
    assert (tmp_path / "x.dna.d").read_bytes() == _lines(reads)
    (tmp_path / "z.fastq.gz").write_bytes(bgzf_util.bgzf(_fastq(inp)))
    r = _harc(["-c", str(tmp_path / "z.fastq.gz"), "-p", "-V", "-t", "2"], _env(HARC_AMD_INGEST_CHUNK="40000"))
    assert r.returncode == 0, r.stdout[-2000:]
    assert _record(tmp_path / "z.harc") == want


def test_the_library_call_writes_the_record_and_the_order_digest_is_the_models(tmp_path):
    import harc_amd
    import torch
    L = 33
    inp = _input(L)
    reads = inp[0]
    fq = _fastq(inp)
    with harc_amd.HarcAmd(harc_amd.default_params(L, num_thr=2)) as h:
        t = torch.frombuffer(bytearray(fq), dtype=torch.uint8).to("cuda")
        torch.cuda.synchronize()
        h.set_fastq_device(t.data_ptr(), len(fq))
        tt = cc.text_digest(_lines(reads))
        assert h.input_order_digest() == tt and tt[1] == N_READS
        sig = h.input_signature()
        h.reorder()
        h.encode()
        assert h.decode_signature() == sig == reads_signature(list(reads))       # what -c -V holds the streams to before it writes them
    (tmp_path / "x.fastq").write_bytes(fq)
    for po in (False, True):
        base = tmp_path / ("b%d" % po)
        (base / "output").mkdir(parents=True)
        harc_amd.compress_fastq(str(tmp_path / "x.fastq"), str(base), L, num_thr=2, num_chains=0, preserve_order=po, check=True)
        rec = cc.parse_check((base / "output" / "read.check").read_bytes())
        assert rec == dict({"reads": reads_signature(list(reads))}, **({"order": cc.order_digest(reads)} if po else {}))
    base = tmp_path / "plain"
    (base / "output").mkdir(parents=True)
    harc_amd.compress_fastq(str(tmp_path / "x.fastq"), str(base), L, num_thr=2, num_chains=0)
    assert not (base / "output" / "read.check").exists()


# ------------------------------------------------------------------------------------------------ what is refused
def _with_members(arc, out, change):
    """the archive with every member that `change` names replaced by change[name](bytes)"""
    with tarfile.open(arc) as t, tarfile.open(out, "w") as o:
        for m in t.getmembers():
            name = m.name[2:] if m.name.startswith("./") else m.name
            if m.isfile() and name in change:
                data = change[name](t.extractfile(m).read())
                m.size = len(data)
                o.addfile(m, io.BytesIO(data))
            else:
                o.addfile(m, t.extractfile(m) if m.isfile() else None)


def _flip_first_rev_bit(tar_bytes):
    """read_rev.tar with one bit of the first byte of read_rev.txt.0 flipped"""
    out = io.BytesIO()
    done = []
    with tarfile.open(fileobj=io.BytesIO(tar_bytes)) as t, tarfile.open(fileobj=out, mode="w") as o:
        for m in t.getmembers():
            if m.isfile() and os.path.basename(m.name) == "read_rev.txt.0":
                data = bytearray(t.extractfile(m).read())
                assert data
                data[0] ^= 1
                done.append(m.name)
                o.addfile(m, io.BytesIO(bytes(data)))
            else:
                o.addfile(m, t.extractfile(m) if m.isfile() else None)
    assert len(done) == 1
    return out.getvalue()


def test_a_changed_stream_byte_decodes_silently_without_V_and_is_refused_with_it(made, tmp_path):
    L = 100
    inp = _input(L)
    reads = inp[0]
    env = _env()
    for name in ("plain", "checked"):
        (tmp_path / name).mkdir()
    (tmp_path / "plain" / "x.fastq").write_bytes(_fastq(inp))
    r = _harc(["-c", str(tmp_path / "plain" / "x.fastq"), "-t", "2"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    shutil.copy(made(L, 0, False) / "x.harc", tmp_path / "checked" / "x.harc")      # the same input with -V
    mp, mv = _flat(_members(tmp_path / "plain" / "x.harc")), _flat(_members(tmp_path / "checked" / "x.harc"))
    assert sorted(mv) == sorted(list(mp) + ["read.check"]) and [k for k in mp if mv[k] != mp[k]] == []       # the two archives differ in read.check only
    for name in ("plain", "checked"):
        _with_members(tmp_path / name / "x.harc", tmp_path / name / "bad.harc", {"read_rev.tar": _flip_first_rev_bit})
    # today's behaviour, and what an archive made without -V still does: status 0 and other reads
    r = _harc(["-d", str(tmp_path / "plain" / "bad.harc")], env)
    assert r.returncode == 0 and "[check]" not in r.stdout, r.stdout[-2000:]
    got = (tmp_path / "plain" / "bad.dna.d").read_bytes().split()
    assert len(got) == len(reads) and sorted(got) != sorted(reads)
    # with the record: refused naming the reads, nothing left
    for mode in ("-d", "-v"):
        r = _harc([mode, str(tmp_path / "checked" / "bad.harc")], env)
        assert r.returncode == 1 and r.stdout.splitlines()[-1].startswith("[check] reads mismatch: recorded "), r.stdout[-2000:]
        assert not (tmp_path / "checked" / "bad.dna.d").exists() and not (tmp_path / "checked" / "output").exists()


def test_the_order_is_checked_apart_from_the_content(made, tmp_path):
    L = 100
    env = _env()
    for name in ("a", "b"):
        (tmp_path / name).mkdir()
    shutil.copy(made(L, 1, False) / "x.harc", tmp_path / "a" / "x.harc")            # -c -p -V of the input
    (tmp_path / "b" / "x.fastq").write_bytes(_fastq(_input(L, True)))               # ... and of the input with two records exchanged
    r = _harc(["-c", str(tmp_path / "b" / "x.fastq"), "-p", "-V", "-t", "2"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    ra, rb = _record(tmp_path / "a" / "x.harc"), _record(tmp_path / "b" / "x.harc")
    assert ra["reads"] == rb["reads"] and ra["order"][0] == rb["order"][0] and ra["order"][1] != rb["order"][1]
    b_check = _members(tmp_path / "b" / "x.harc")["read.check"]
    _with_members(tmp_path / "a" / "x.harc", tmp_path / "a" / "mix.harc", {"read.check": lambda _: b_check})      # A's streams, B's record
    for mode in ("-d", "-v"):
        r = _harc([mode, str(tmp_path / "a" / "mix.harc"), "-p"], env)
        last = r.stdout.splitlines()[-1]
        assert r.returncode == 1 and last.startswith("[check] order mismatch: recorded ") and "reads" not in last, r.stdout[-2000:]
        assert not (tmp_path / "a" / "mix.dna.d").exists() and not (tmp_path / "a" / "output").exists()
    r = _harc(["-d", str(tmp_path / "a" / "mix.harc")], env)
    assert r.returncode == 0 and _check_line(r.stdout).startswith("[check] reads ok, order not checked (no -p)"), r.stdout[-2000:]


def test_a_changed_side_file_is_refused_naming_it(made, tmp_path):
    L = 33
    env = _env()
    for f in ("x.harc", "x.quality", "x.id"):                       # what -c -p -q -V left
        shutil.copy(made(L, 2, False) / f, tmp_path / f)
    q, i = (tmp_path / "x.quality").read_bytes(), (tmp_path / "x.id").read_bytes()
    bad = bytearray(q)
    bad[len(q) // 2] = bad[len(q) // 2] ^ 1 if bad[len(q) // 2] != 10 else 11
    (tmp_path / "x.quality").write_bytes(bytes(bad))
    r = _harc(["-d", str(tmp_path / "x.harc"), "-p", "-q"], env)
    assert r.returncode == 1 and r.stdout.splitlines()[-1].startswith("[check] quality mismatch: recorded "), r.stdout[-2000:]
    assert not (tmp_path / "x.d.fastq").exists() and not (tmp_path / "output").exists()
    (tmp_path / "x.quality").write_bytes(q)
    lines = i.split(b"\n")
    assert lines[5] != lines[1500] and len(lines[5]) == len(lines[1500])
    lines[5], lines[1500] = lines[1500], lines[5]
    (tmp_path / "x.id").write_bytes(b"\n".join(lines))
    r = _harc(["-d", str(tmp_path / "x.harc"), "-p", "-q"], env)
    assert r.returncode == 1 and r.stdout.splitlines()[-1].startswith("[check] ids mismatch: recorded "), r.stdout[-2000:]
    assert not (tmp_path / "x.d.fastq").exists() and not (tmp_path / "output").exists()
