"""Paired-end input on the GPU.  Library level: harc_amd.compress_fastq_pair(A, B) leaves, file by file, what harc_amd.compress_fastq leaves on `cat A B` with
the same build and the same (K, S) -- with each file in one piece and in several, plain and BGZF in every mix -- and refuses what a pair run must not
tolerate.  Command line: ./harc -c A -2 B -p -q -I -Q -S -V followed by ./harc -d -p -q gives both files back byte for byte under every mate rule, gzipped
too, in pieces of a few lines too; a rule that is not the recorded one is refused by the count of the patch kernel."""
import functools
import gzip
import io
import os
import random
import shutil
import subprocess
import tarfile

import pytest

from tests import bgzf_util as bu
from tests import idmate_cases as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, S, E = 4, 16, 2
SHAPES = [(3001, 100), (1, 100), (257, 63)]
STYLES = ("space", "slash", "same", "none")


def _mate_ids(n, style):
    if style == "space":
        return mc.illumina_pairs(n)
    if style == "slash":
        return mc.slash_pairs(n)
    if style == "same":
        return mc.sra_pairs(n)
    a, b = mc.illumina_pairs(n)
    b = list(b)
    random.Random(3).shuffle(b)
    if n == 1:
        b[0] = b[0] + b"x"
    return a, tuple(b)


@functools.lru_cache(maxsize=None)
def _pair(n, L, style="space"):
    """two FASTQ files of n records of L bases, reads with N among them, with mate ids in `style`"""
    out = []
    for k, ids in enumerate(_mate_ids(n, style)):
        rec = bu.fastq_text(n, L, seed=21 + k).split(b"\n")
        rec[0:4 * n:4] = ids
        out.append(b"\n".join(rec))
    return tuple(out)


def _files(d):
    return {f: (d / f).read_bytes() for f in sorted(os.listdir(d)) if (d / f).is_file()}


@functools.lru_cache(maxsize=None)
def _cat_run(n, L, root):
    """what compress_fastq leaves on `cat A B`, computed once per shape"""
    import harc_amd
    a, b = _pair(n, L)
    d = root / ("cat_%d_%d" % (n, L))
    os.makedirs(d / "output")
    (d / "c.fastq").write_bytes(a + b)
    harc_amd.compress_fastq(str(d / "c.fastq"), str(d), L, num_thr=E, num_chains=K, num_steps=S, preserve_order=True, preserve_quality=True)
    return _files(d / "output")


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("pair")


# (a file of one record is one piece: no "pieces" variants for it)
@pytest.mark.parametrize("n, L, variant", [(n, L, v) for n, L in SHAPES for v in ("plain", "pieces", "plain_bgzf", "bgzf_bgzf_pieces") if n > 1 or "pieces" not in v])
def test_the_pair_call_leaves_what_the_cat_run_leaves(n, L, variant, root, tmp_path, monkeypatch, oracle):
    import harc_amd
    a, b = _pair(n, L)
    want = _cat_run(n, L, root)
    if "pieces" in variant:
        # each file at least three pieces: FASTQ bytes per piece, or compressed bytes for BGZF
        size = len(bu.bgzf(a, member_text=3000)) if "bgzf" in variant else len(a)
        monkeypatch.setenv("HARC_AMD_INGEST_CHUNK", str(size // 4))
    fa, fb = tmp_path / "a.fastq", tmp_path / "b.fastq"
    fa.write_bytes(bu.bgzf(a, member_text=3000) if variant.startswith("bgzf") else a)
    fb.write_bytes(bu.bgzf(b, member_text=3000) if "bgzf" in variant else b)
    os.makedirs(tmp_path / "output")
    got_n = harc_amd.compress_fastq_pair(str(fa), str(fb), str(tmp_path), L, num_thr=E, num_chains=K, num_steps=S, preserve_quality=True)
    assert got_n == n
    got = _files(tmp_path / "output")
    assert got.pop("read.pair") == b"HARCP1\nrecords %d\n" % n
    id2 = got.pop("output.id2")
    assert got["output.id"] + id2 == want["output.id"]
    assert got["output.id"] == b"".join(x + b"\n" for x in a.split(b"\n")[0:4 * n:4])
    got["output.id"] = want["output.id"]
    assert sorted(got) == sorted(want)
    for f in want:                                                 # read_order_N.bin, output.quality and every stream among them
        assert got[f] == want[f], f
    if variant == "plain" and n == SHAPES[0][0]:                  # ... and the streams decode to the reads of both files under the CPU oracle
        assert oracle.harc_oracle_decoder(str(tmp_path).encode(), E) == 0
        reads = (a + b).split(b"\n")[1::4]
        assert sorted((tmp_path / "output" / "output.dna").read_bytes().split()) == sorted(reads)


def test_the_pair_call_without_quality_and_with_check(tmp_path):
    import harc_amd
    n, L = 257, 63
    a, b = _pair(n, L)
    (tmp_path / "a.fastq").write_bytes(a)
    (tmp_path / "b.fastq").write_bytes(b)
    os.makedirs(tmp_path / "output")
    assert harc_amd.compress_fastq_pair(str(tmp_path / "a.fastq"), str(tmp_path / "b.fastq"), str(tmp_path), L, num_thr=E, num_chains=K, num_steps=S, check=True) == n
    got = _files(tmp_path / "output")
    assert "output.id" not in got and "output.id2" not in got and "output.quality" not in got
    rec = got["read.check"].decode().splitlines()
    assert rec[0] == "HARCV1" and rec[1].startswith("reads %016x " % (2 * n)) and rec[2].startswith("order %016x " % (2 * n * (L + 1))), rec


@pytest.mark.parametrize("what", ["unequal_counts", "a_without_final_newline", "a_ends_after_line_2", "b_ends_after_line_3", "different_read_lengths"])
def test_the_pair_call_refuses(what, tmp_path):
    import harc_amd
    n, L = 257, 63
    a, b = _pair(n, L)
    words = {"unequal_counts": "different numbers of records", "a_without_final_newline": "a.fastq does not end in a newline",
             "a_ends_after_line_2": "a.fastq does not hold whole 4-line records", "b_ends_after_line_3": "b.fastq does not hold whole 4-line records",
             "different_read_lengths": "read length not fixed"}[what]
    if what == "unequal_counts":
        b = b"\n".join(b.split(b"\n")[:4 * (n - 1)]) + b"\n"
    elif what == "a_without_final_newline":
        a = a[:-1]
    elif what == "a_ends_after_line_2":
        a = b"\n".join(a.split(b"\n")[:4 * (n - 1) + 2]) + b"\n"
    elif what == "b_ends_after_line_3":
        b = b"\n".join(b.split(b"\n")[:4 * (n - 1) + 3]) + b"\n"
    else:
        b = _pair(n, 100)[1]
    (tmp_path / "a.fastq").write_bytes(a)
    (tmp_path / "b.fastq").write_bytes(b)
    os.makedirs(tmp_path / "output")
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.compress_fastq_pair(str(tmp_path / "a.fastq"), str(tmp_path / "b.fastq"), str(tmp_path), L, num_thr=E, num_chains=K, num_steps=S, preserve_quality=True)
    assert e.value.code == -1 and words in str(e.value), str(e.value)
    if what == "unequal_counts":
        assert "%d" % n in str(e.value) and "%d" % (n - 1) in str(e.value)
    left = os.listdir(tmp_path / "output")
    assert not [f for f in left if f.startswith("read") or f.endswith(".bin") or f.endswith(".dna")], left      # nothing of an archive


# ------------------------------------------------------------------------------------------------ the files of the restore, in process
def _side_files(d, a, b, n, rule):
    """what the decoder and -c -q leave for fastq_assemble_pair: the reads and quality values of both files, the ids folded unless the rule is none"""
    la, lb = a.split(b"\n"), b.split(b"\n")
    join = lambda x: b"".join(y + b"\n" for y in x)
    (d / "x.dna").write_bytes(join(la[1:4 * n:4] + lb[1:4 * n:4]))
    (d / "x.quality").write_bytes(join(la[3:4 * n:4] + lb[3:4 * n:4]))
    (d / "x.id").write_bytes(join(la[0:4 * n:4] + (lb[0:4 * n:4] if rule == "none" else [])))


@pytest.mark.parametrize("piece", [None, 150, 47])
@pytest.mark.parametrize("style", STYLES)
def test_assemble_pair_in_pieces_of_a_few_lines(style, piece, tmp_path, monkeypatch):
    """150 and 47 bytes: a piece holds three id lines or none whole; on the none path the cut between file 1 and file 2 falls inside a piece, on the others
    a patched line is a piece's last whole line and what is carried is patched a piece later"""
    import harc_amd
    n, L = 300, 63
    a, b = _pair(n, L, style)
    _side_files(tmp_path, a, b, n, style)
    if piece:
        monkeypatch.setenv("HARC_AMD_FQOUT_PIECE", str(piece))
    for bgzf in (False, True):
        o1, o2 = tmp_path / ("1.%d" % bgzf), tmp_path / ("2.%d" % bgzf)
        harc_amd.fastq_assemble_pair(str(tmp_path / "x.dna"), str(tmp_path / "x.id"), str(tmp_path / "x.quality"), str(o1), str(o2), n, style, bgzf=bgzf)
        if bgzf:
            assert o1.read_bytes() == harc_amd.bgzf_deflate_host(a) and o2.read_bytes() == harc_amd.bgzf_deflate_host(b)
        else:
            assert o1.read_bytes() == a and o2.read_bytes() == b


def test_assemble_pair_refuses_a_wrong_rule_and_wrong_counts(tmp_path):
    import harc_amd
    n, L = 300, 63
    a, b = _pair(n, L, "slash")
    _side_files(tmp_path, a, b, n, "slash")
    o1, o2 = tmp_path / "o1", tmp_path / "o2"
    args = [str(tmp_path / "x.dna"), str(tmp_path / "x.id"), str(tmp_path / "x.quality"), str(o1), str(o2)]
    for rule, count, words in (("space", n, "do not carry the '1'"), ("none", n, "%d lines, %d are needed" % (n, 2 * n)), ("slash", n - 1, "2 x %d" % (n - 1))):
        with pytest.raises(harc_amd.HarcAmdError) as e:
            harc_amd.fastq_assemble_pair(*args, count, rule)
        assert e.value.code == -1 and words in str(e.value), str(e.value)
        assert not o1.exists() and not o2.exists()
    _side_files(tmp_path, a, b, n, "none")                          # 2 n id lines where a rule promises n
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.fastq_assemble_pair(*args, n, "slash")
    assert "%d lines, %d are needed" % (2 * n, n) in str(e.value) and not o1.exists() and not o2.exists()
    # the one-file call is what it was
    harc_amd.fastq_assemble(*args[:4])
    assert o1.read_bytes() == a + b


# ------------------------------------------------------------------------------------------------ the command line
def _harc(args, env=None):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


@functools.lru_cache(maxsize=None)
def _archive(style, root):
    """./harc -c A -2 B -p -q -I -Q -S -V, once per id style -> the directory with s_1.harc, s_1.id.hi and s_1.quality.hq"""
    n, L = 300, 100
    a, b = _pair(n, L, style)
    d = root / ("cli_" + style)
    d.mkdir()
    (d / "s_1.fastq").write_bytes(a)
    (d / "s_2.fastq").write_bytes(b)
    env = {k: v for k, v in os.environ.items() if k != "HARC_AMD_STAGE3"}
    r = subprocess.run([os.path.join(ROOT, "harc"), "-c", str(d / "s_1.fastq"), "-2", str(d / "s_2.fastq"), "-p", "-q", "-I", "-Q", "-S", "-V", "-t", "2"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert (d / "s_1.harc").exists() and not (d / "output").exists() and not (d / "s_1.id").exists() and not (d / "s_2.harc").exists()
    with tarfile.open(d / "s_1.harc") as t:
        assert t.extractfile("./read.pair").read() == b"HARCP1\nrecords %d\nids %s\n" % (n, style.encode())
        assert not [m.name for m in t.getmembers() if "id2" in m.name]
    return d, a, b


@pytest.mark.parametrize("style", STYLES)
def test_harc_roundtrip_of_a_pair_under_every_rule(style, root):
    d, a, b = _archive(style, root)
    r = _harc(["-d", str(d / "s_1.harc"), "-p", "-q"])
    assert r.returncode == 0, r.stdout[-3000:]
    assert "[check] reads ok, order ok, ids ok, quality ok" in r.stdout, r.stdout[-3000:]
    assert (d / "s_1.d.1.fastq").read_bytes() == a and (d / "s_1.d.2.fastq").read_bytes() == b
    assert not (d / "output").exists() and not (d / "s_1.d.fastq").exists()


@pytest.mark.parametrize("style", ["space", "none"])
def test_harc_d_z_writes_each_file_as_the_bgzf_of_its_text(style, root):
    import harc_amd
    d, a, b = _archive(style, root)
    r = _harc(["-d", str(d / "s_1.harc"), "-p", "-q", "-z"], {"HARC_AMD_FQOUT_PIECE": "700"})
    assert r.returncode == 0, r.stdout[-3000:]
    g1, g2 = (d / "s_1.d.1.fastq.gz").read_bytes(), (d / "s_1.d.2.fastq.gz").read_bytes()
    assert gzip.decompress(g1) == a and gzip.decompress(g2) == b
    assert g1 == harc_amd.bgzf_deflate_host(a) and g2 == harc_amd.bgzf_deflate_host(b)


def test_harc_v_passes_and_other_modes_on_a_paired_archive(root):
    d, a, b = _archive("space", root)
    r = _harc(["-v", str(d / "s_1.harc"), "-p", "-q"])
    assert r.returncode == 0 and "[check] reads ok, order ok, ids ok, quality ok" in r.stdout, r.stdout[-3000:]
    r = _harc(["-d", str(d / "s_1.harc"), "-p"])
    assert r.returncode == 0, r.stdout[-3000:]
    assert (d / "s_1.dna.d").read_bytes() == b"".join(x + b"\n" for x in (a + b).split(b"\n")[1::4])      # file 1's reads, then file 2's
    r = _harc(["-d", str(d / "s_1.harc"), "-q"])
    assert r.returncode == 1 and "-q needs -p on an archive of a pair" in r.stdout and not (d / "output").exists(), r.stdout[-3000:]


def test_harc_refuses_a_flipped_rule_by_the_count_of_the_patch_kernel(root, tmp_path):
    d, a, b = _archive("slash", root)
    for f in ("s_1.id.hi", "s_1.quality.hq"):
        shutil.copy(d / f, tmp_path / f)
    with tarfile.open(d / "s_1.harc") as t, tarfile.open(tmp_path / "s_1.harc", "w") as o:
        for m in t.getmembers():
            if m.name == "./read.pair":
                data = t.extractfile(m).read().replace(b"ids slash", b"ids space")
                m.size = len(data)
                o.addfile(m, io.BytesIO(data))
            else:
                o.addfile(m, t.extractfile(m) if m.isfile() else None)
    r = _harc(["-d", str(tmp_path / "s_1.harc"), "-p", "-q"])
    assert r.returncode == 1 and "do not carry the '1'" in r.stdout and "space" in r.stdout, r.stdout[-3000:]
    assert not (tmp_path / "s_1.d.1.fastq").exists() and not (tmp_path / "s_1.d.2.fastq").exists() and not (tmp_path / "output").exists()


def test_harc_refuses_files_of_different_record_counts_and_leaves_nothing(tmp_path):
    n, L = 257, 63
    a, b = _pair(n, L)
    (tmp_path / "s_1.fastq").write_bytes(a)
    (tmp_path / "s_2.fastq").write_bytes(b"\n".join(b.split(b"\n")[:4 * (n - 1)]) + b"\n")
    r = _harc(["-c", str(tmp_path / "s_1.fastq"), "-2", str(tmp_path / "s_2.fastq"), "-p", "-q"], {"HARC_AMD_STAGE3": "none"})
    assert r.returncode == 1 and "different numbers of records" in r.stdout and "%d" % n in r.stdout and "%d" % (n - 1) in r.stdout, r.stdout[-3000:]
    assert not (tmp_path / "output").exists() and not (tmp_path / "s_1.harc").exists() and not (tmp_path / "s_1.id").exists()
