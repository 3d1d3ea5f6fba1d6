"""Match by sequence on the GPU (./harc -d -M MOTIFS [-e K]; README: "-M and what it promises").  The device call against the plain-Python restatement of
tests/match_cases.py on every case, with the reads at each of the 16 alignments of a device address among bytes that would match if they were read; the file call in
pieces of 1, 3 and 7 lines and the default, without side files, with them, and on the layouts of a pair; and ./harc end to end, where every result is the
restatement's filter of what the same command without -M writes."""
import functools
import gzip
import os
import subprocess

import pytest

from tests import bgzf_out_cases as oc
from tests import gen
from tests import idmate_cases as mc
from tests import match_cases as tc
from tests import quality_cases as qc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = tc.cases()
L = 100


@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        yield h


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("match")


def _on_device(b, lead, fill=0x41, tail=64):
    """b at `lead` bytes behind the start of an allocation -> (tensor, device address of b); the bytes around it are `fill`"""
    import torch
    t = torch.full((lead + len(b) + tail,), fill, dtype=torch.uint8, device="cuda")
    if b:
        t[lead:lead + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()                                          # the library works on a stream of its own
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + lead


def _flags_device(ctx, c, lead):
    text = tc.text_of(c["reads"])
    n = len(c["reads"])
    tt, pt = _on_device(text, lead)
    tf, pf = _on_device(b"\x55" * n, 3, fill=0x77)
    hits, found = ctx.motif_flags_device(c["motifs"], pt, n, c["L"], pf, c["k"])
    raw = bytes(tf.cpu().numpy().tobytes())
    assert raw[:3] == b"\x77" * 3 and raw[3 + n:] == b"\x77" * 64, "bytes around the flags were written"
    return raw[3:3 + n], hits, found


# ------------------------------------------------------------------------------------------------ the device call
@pytest.mark.parametrize("name", sorted(CASES))
def test_motif_flags_device_equals_the_restatement(ctx, name):
    c = CASES[name]
    for lead in (0, 5):
        flags, hits, found = _flags_device(ctx, c, lead)
        assert flags == c["flags"], (name, lead, [i for i in range(len(flags)) if flags[i] != c["flags"][i]][:10])
        assert hits == c["hits"] and found == sum(c["hits"]), (name, lead)


@pytest.mark.parametrize("lead", range(16))
def test_the_text_at_each_of_the_16_alignments(ctx, lead):
    """the first and the last line carry the motif at their first and last offset, and the bytes in front of and behind the text are 'A': with the motif AAAA..
    a load that took them for the text would flag the lines next to them"""
    for Lr in (21, 100):
        p = b"A" * 8
        reads = [p + b"C" * (Lr - 8), b"C" * Lr, b"C" * (Lr - 7) + b"A" * 7, b"A" * 7 + b"C" * (Lr - 7), b"C" * Lr, b"C" * (Lr - 8) + p]
        c = tc._case(p + b"\n", reads)
        assert c["flags"] == b"\1\0\0\0\0\1"
        flags, hits, found = _flags_device(ctx, c, lead)
        assert flags == c["flags"] and hits == b"\1", (Lr, lead)
        c = tc._case(p + b"\n", reads[1:5])
        flags, hits, found = _flags_device(ctx, c, lead)
        assert flags == b"\0\0\0\0" and hits == b"\0" and found == 0, (Lr, lead)


def test_motif_flags_device_is_what_the_host_twin_gives(ctx):
    import harc_amd
    for name in ("random_2000", "random_300_K2", "lengths_L255", "n_handling_K1"):
        c = CASES[name]
        flags, hits, found = _flags_device(ctx, c, 9)
        assert (flags, hits, found) == harc_amd.motif_flags_host(c["motifs"], tc.text_of(c["reads"]), c["L"], c["k"]), name


def test_the_random_case_cannot_pass_on_all_zero_or_all_one_flags(ctx):
    c = CASES["random_2000"]
    flags, hits, found = _flags_device(ctx, c, 1)
    assert 0 < sum(flags) < len(flags) and found == 3 and len(hits) == 4 and flags == c["flags"]


def test_motif_flags_device_refuses_what_the_rule_refuses(ctx):
    import harc_amd
    tt, pt = _on_device(b"ACGT\n", 0)
    tf, pf = _on_device(b"\0", 0)
    for text, k, line in tc.refusals()[:8]:
        with pytest.raises(harc_amd.HarcAmdError, match="line %d:" % line):
            ctx.motif_flags_device(text, pt, 1, 4, pf, k)
    with pytest.raises(harc_amd.HarcAmdError, match="read length"):
        ctx.motif_flags_device(b"ACGT\n", pt, 1, 256, pf)
    assert ctx.motif_flags_device(b"ACGT\n", 0, 0, 4, 0) == (b"\0", 0)


# ------------------------------------------------------------------------------------------------ the file call
def _job(n, pair=None):
    """reads of 24 that tell their record, quality values that do too, ids whose lines differ in length; pair: 'space' or 'none' -> the job of 2 n records"""
    total = 2 * n if pair else n
    reads = [b"C" * 24 for _ in range(total)]
    quality = b"".join(b"%023dI\n" % i for i in range(total))
    ids = [b"@r%d%s len=%d" % (i, b"x" * (i * 5 % 23), i) for i in range(n)]
    if pair == "none":
        ids = ids + [b"@m%d/2 mate" % i for i in range(n)]
    return ids, reads, quality


def _match_files(tmp_path, motifs, reads, ids=None, quality=None, **kw):
    import harc_amd
    (tmp_path / "m").write_bytes(motifs)
    (tmp_path / "d").write_bytes(tc.text_of(reads))
    if ids is not None:
        (tmp_path / "i").write_bytes(tc.text_of(ids))
        (tmp_path / "q").write_bytes(quality)
    for name in ("oi", "od", "oq"):
        if (tmp_path / name).exists():
            os.remove(tmp_path / name)
    p = lambda x: str(tmp_path / x)
    if ids is None:
        st = harc_amd.match_files(p("m"), p("d"), p("od"), **kw)
        assert not (tmp_path / "oi").exists() and not (tmp_path / "oq").exists()
        return st, (tmp_path / "od").read_bytes()
    st = harc_amd.match_files(p("m"), p("d"), p("od"), p("i"), p("q"), p("oi"), p("oq"), **kw)
    return st, tuple((tmp_path / x).read_bytes() for x in ("oi", "od", "oq"))


P1, P2, ABSENT = b"AGATCGGAAGAGC", b"TTAGGCATTAGG", b"GGAGGAGGAGGAGG"


@pytest.mark.parametrize("lines", ["1", "3", "7", None])
def test_match_files_in_pieces_gives_the_same_files(tmp_path, monkeypatch, lines):
    if lines:
        monkeypatch.setenv("HARC_AMD_MATCH_LINES", lines)
        monkeypatch.setenv("HARC_AMD_SELECT_LINES", lines)
        monkeypatch.setenv("HARC_AMD_SELECT_PIECE", "97")
    n = 41
    ids, reads, quality = _job(n)
    motifs = P1 + b"\n>absent\n" + ABSENT + b"\n" + P2.lower() + b"\n"
    # matched: the first and the last read, neighbours, on both strands, one with a mismatch that K = 1 takes
    for i, q in ((0, P1), (6, P2), (7, tc.rc(P1)), (8, P1), (20, tc.rc(P2)), (n - 1, P2)):
        reads[i] = tc._plant(reads[i], (3 * i) % 11, q)
    reads[30] = tc._plant(reads[30], 5, tc._with_mismatches(P1, [4]))
    for k, sel in ((0, [0, 6, 7, 8, 20, n - 1]), (1, [0, 6, 7, 8, 20, 30, n - 1])):
        want, hits = tc.flags_hits(tc.parse(motifs, k), reads, k)
        assert [i for i in range(n) if want[i]] == sel and hits == b"\1\0\1"
        # the reads alone
        st, od = _match_files(tmp_path, motifs, reads, k=k)
        assert st == (3, 2, len(sel), n, [ABSENT]) and od == tc.gather(reads, want), (lines, k)
        # with the text side files
        st, (oi, od, oq) = _match_files(tmp_path, motifs, reads, ids, quality, k=k)
        assert st == (3, 2, len(sel), n, [ABSENT]), (lines, k)
        assert oi == tc.gather(ids, want) and od == tc.gather(reads, want) and oq == tc.gather(quality.split(b"\n")[:-1], want), (lines, k)


@pytest.mark.parametrize("lines", ["3", None])
def test_match_files_on_the_layouts_of_a_pair(tmp_path, monkeypatch, lines):
    if lines:
        monkeypatch.setenv("HARC_AMD_MATCH_LINES", lines)
        monkeypatch.setenv("HARC_AMD_SELECT_LINES", lines)
        monkeypatch.setenv("HARC_AMD_SELECT_PIECE", "61")
    n = 17
    motifs = P1 + b"\n" + P2 + b"\n"
    for rule in ("slash", "none"):
        ids, reads, quality = _job(n, rule)
        # pair 3 by its first mate, pair 5 by its second mate only, pair 16 by both, pair 0 by the reverse strand of its second mate
        for i, q in ((3, P1), (n + 5, P2), (16, P1), (n + 16, P2), (n + 0, tc.rc(P1))):
            reads[i] = tc._plant(reads[i], i % 9, q)
        half, hits = tc.flags_hits(tc.parse(motifs), reads)
        assert [i for i in range(2 * n) if half[i]] == [3, 16, n, n + 5, n + 16]
        f = bytes(half[i] | half[n + i] for i in range(n))
        st, (oi, od, oq) = _match_files(tmp_path, motifs, reads, ids, quality, pair_records=n, pair_rule=rule)
        assert st == (2, 2, 4, n, []), (rule, lines)
        assert oi == tc.gather(ids, f + f if rule == "none" else f), (rule, lines)      # folded ids: file 1's lines, once
        assert od == tc.gather(reads, f + f) and oq == tc.gather(quality.split(b"\n")[:-1], f + f), (rule, lines)


def test_match_files_of_nothing_gives_empty_files(tmp_path):
    ids, reads, quality = _job(9)
    st, outs = _match_files(tmp_path, P1 + b"\n", reads, ids, quality)
    assert st == (1, 0, 0, 9, [P1]) and outs == (b"", b"", b"")
    st, od = _match_files(tmp_path, P1 + b"\n", reads)
    assert st == (1, 0, 0, 9, [P1]) and od == b""
    st, od = _match_files(tmp_path, b"C" * 25 + b"\n", reads)         # a motif longer than the reads matches nothing: not an error
    assert st == (1, 0, 0, 9, [b"C" * 25]) and od == b""


def test_match_files_refuses_what_does_not_fit_and_leaves_no_output(tmp_path):
    import harc_amd
    ids, reads, quality = _job(9)
    reads[2] = tc._plant(reads[2], 1, P1)
    cases = [
        (dict(motifs=b"ACGT\r\n"), {}, "line 1: byte 0x0d"),
        (dict(motifs=b""), {}, "is empty"),
        (dict(motifs=P1 + b"\n"), dict(k=13), "line 1: .* every window would match|K = 13"),
        (dict(ids=ids[:-1]), {}, "holds 8 lines, 9 are wanted"),
        (dict(ids=ids + [b"@one more"]), {}, "holds 10 lines, 9 are wanted"),
        (dict(quality=quality + b"%023dI\n" % 9), {}, "holds 250 bytes, .* 225"),
        (dict(), dict(pair_records=4, pair_rule="slash"), "a pair of 4 records is wanted, .* holds 9 reads"),
    ]
    for texts, kw, words in cases:
        t = dict(motifs=P1 + b"\n", ids=ids, quality=quality)
        t.update(texts)
        with pytest.raises(harc_amd.HarcAmdError, match=words) as e:
            _match_files(tmp_path, t["motifs"], reads, t["ids"], t["quality"], **kw)
        assert e.value.code == -1, str(e.value)
        assert not any((tmp_path / x).exists() for x in ("oi", "od", "oq")), words
    with pytest.raises(harc_amd.HarcAmdError, match="a pair is two FASTQ files"):
        _match_files(tmp_path, P1 + b"\n", reads, pair_records=4, pair_rule="slash")


# ------------------------------------------------------------------------------------------------ the command line
def _harc(args, env=None):
    e = dict(os.environ, HARC_AMD_STAGE3="none")
    e.update(env or {})
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _fastq(n, seed, ids=None):
    reads = gen.reads_text(seed, n, L, 15000, err=0.01, n_frac=0.02).split()
    quals = qc.markov(n, L, seed=seed).split()
    ids = ids or oc.illumina_text(n).split(b"\n")[0:-1:4]
    return b"".join(b"%s\n%s\n+\n%s\n" % (i, r, q) for i, r, q in zip(ids, reads, quals))


def _left(d, stem):
    """what a restore has written next to the archive"""
    return sorted(f for f in os.listdir(d) if f.startswith(stem + ".") and (".d." in f or f.endswith(".dna.d"))) + (["output"] if (d / "output").exists() else [])


@functools.lru_cache(maxsize=None)
def _archive(kind, root):
    """./harc -c, once per kind of archive -> (its directory, the FASTQ text or the two texts of a pair)"""
    d = root / kind
    d.mkdir()
    if kind == "pair":
        a_ids, b_ids = mc.slash_pairs(300)
        fq = _fastq(300, 85, list(a_ids)), _fastq(300, 86, list(b_ids))
        (d / "x.fastq").write_bytes(fq[0])
        (d / "x_2.fastq").write_bytes(fq[1])
        r = _harc(["-c", str(d / "x.fastq"), "-2", str(d / "x_2.fastq"), "-p", "-q", "-t", "2"])
        assert r.returncode == 0 and (d / "x.id").exists(), r.stdout[-3000:]
        return d, fq
    fq = _fastq(400, 81)
    (d / "x.fastq").write_bytes(fq)
    flags = {"plain": ["-p", "-q"], "packed": ["-p", "-q", "-Q", "-I", "-V"], "stored": ["-q"]}[kind]
    r = _harc(["-c", str(d / "x.fastq")] + flags + ["-t", "2"], {"HARC_AMD_QPACK_BLOCK": "256", "HARC_AMD_IDPACK_BLOCK": "512"})
    assert r.returncode == 0 and (d / "x.harc").exists(), r.stdout[-3000:]
    return d, fq


def _motifs_of(fq):
    """three windows of reads of the text, one of them given as its reverse complement and in lower case, and a motif that occurs nowhere"""
    reads = [r for r in tc.fastq_reads(fq) if b"N" not in r]
    return b">from the reads\n" + reads[3][10:34] + b"\n" + tc.rc(reads[50][60:90]).lower() + b"\n" + reads[120][0:22] + b"\n>nowhere\n" + b"ACGTTGCA" * 4 + b"\n"


def _want(fq, motifs, k):
    ms = tc.parse(motifs, k)
    flags, hits = tc.flags_hits(ms, tc.fastq_reads(fq), k)
    return flags, hits, ms


@pytest.mark.parametrize("kind", ["plain", "packed"])
def test_harc_matches_by_sequence_plain_and_gzipped(kind, root):
    import harc_amd
    d, fq = _archive(kind, root)
    motifs = _motifs_of(fq)
    (d / "motifs.txt").write_bytes(motifs)
    n = fq.count(b"\n") // 4
    for k in (0, 1):
        flags, hits, ms = _want(fq, motifs, k)
        sel = sum(flags)
        assert 2 < sel < n / 4 and hits == b"\1\1\1\0"
        r = _harc(["-d", str(d / "x.harc"), "-p", "-q", "-M", str(d / "motifs.txt"), "-e", str(k)], {"HARC_AMD_MATCH_LINES": "64", "HARC_AMD_SELECT_LINES": "100"})
        assert r.returncode == 0, r.stdout[-3000:]
        assert (d / "x.hit.d.fastq").read_bytes() == tc.filter_fastq(fq, flags), k
        assert "[match] 4 motifs, 3 found, %d of %d records" % (sel, n) in r.stdout and "[match] not found: " + "ACGTTGCA" * 4 in r.stdout, r.stdout[-3000:]
        if kind == "packed":                                          # the archive of -V is checked whole, in front of the match
            assert "[check] reads ok, order ok, ids ok, quality ok" in r.stdout and r.stdout.index("[check]") < r.stdout.index("[match]"), r.stdout[-3000:]
    assert _left(d, "x") == ["x.hit.d.fastq"]
    if kind == "packed":
        return                                                        # (-z goes through the same unchanged assembly)
    flags, hits, ms = _want(fq, motifs, 0)
    r = _harc(["-d", str(d / "x.harc"), "-p", "-q", "-z", "-M", str(d / "motifs.txt")])
    assert r.returncode == 0, r.stdout[-3000:]
    gz = (d / "x.hit.d.fastq.gz").read_bytes()
    assert gzip.decompress(gz) == tc.filter_fastq(fq, flags) and gz == harc_amd.bgzf_deflate_host(tc.filter_fastq(fq, flags))
    # without -q: the reads' lines alone
    r = _harc(["-d", str(d / "x.harc"), "-p", "-M", str(d / "motifs.txt")])
    assert r.returncode == 0, r.stdout[-3000:]
    assert (d / "x.hit.dna.d").read_bytes() == tc.gather(tc.fastq_reads(fq), flags)
    assert _left(d, "x") == ["x.hit.d.fastq", "x.hit.d.fastq.gz", "x.hit.dna.d"]      # a hit never stands in for a full restore, and output/ is gone


def test_harc_matches_pairs_and_keeps_mates_together(root):
    d, (a, b) = _archive("pair", root)
    ra, rb = tc.fastq_reads(a), tc.fastq_reads(b)
    clean = [i for i in range(len(rb)) if b"N" not in rb[i]]
    motifs = ra[[i for i in range(len(ra)) if b"N" not in ra[i]][2]][5:31] + b"\n" + tc.rc(rb[clean[7]][40:70]) + b"\n"
    (d / "motifs.txt").write_bytes(motifs)
    fa, _, ms = _want(a, motifs, 0)
    fb, _, _ = _want(b, motifs, 0)
    both = bytes(x | y for x, y in zip(fa, fb))
    assert any(y and not x for x, y in zip(fa, fb)) and 1 < sum(both) < 100      # a pair selected by its second mate only
    r = _harc(["-d", str(d / "x.harc"), "-p", "-q", "-M", str(d / "motifs.txt")], {"HARC_AMD_MATCH_LINES": "50", "HARC_AMD_SELECT_LINES": "64"})
    assert r.returncode == 0, r.stdout[-3000:]
    assert (d / "x.hit.d.1.fastq").read_bytes() == tc.filter_fastq(a, both)
    assert (d / "x.hit.d.2.fastq").read_bytes() == tc.filter_fastq(b, both)
    assert "%d of 300 records" % sum(both) in r.stdout, r.stdout[-3000:]
    assert _left(d, "x") == ["x.hit.d.1.fastq", "x.hit.d.2.fastq"]
    # without -q the archive of a pair is the plain X.dna.d of 2 n lines, filtered line by line
    r = _harc(["-d", str(d / "x.harc"), "-p", "-M", str(d / "motifs.txt")])
    assert r.returncode == 0 and "%d of 600 records" % (sum(fa) + sum(fb)) in r.stdout, r.stdout[-3000:]
    assert (d / "x.hit.dna.d").read_bytes() == tc.gather(ra + rb, fa + fb)


def test_harc_matches_in_stored_order_without_p(root):
    d, fq = _archive("stored", root)
    motifs = _motifs_of(fq)
    (d / "motifs.txt").write_bytes(motifs)
    r = _harc(["-d", str(d / "x.harc"), "-q"])
    assert r.returncode == 0, r.stdout[-3000:]
    full = (d / "x.d.fastq").read_bytes()
    os.remove(d / "x.d.fastq")
    flags, hits, ms = _want(full, motifs, 2)
    r = _harc(["-d", str(d / "x.harc"), "-q", "-M", str(d / "motifs.txt"), "-e", "2"])
    assert r.returncode == 0, r.stdout[-3000:]
    assert (d / "x.hit.d.fastq").read_bytes() == tc.filter_fastq(full, flags) and sum(flags) > 2      # a filter of what the full restore writes, in its order


def test_harc_a_list_that_matches_nothing_is_status_1_and_writes_nothing(root):
    d, fq = _archive("plain", root)
    before = _left(d, "x")
    (d / "nothing.txt").write_bytes(b"ACGTTGCA" * 4 + b"\n" + b"A" * 101 + b"\n")
    for args in (["-p", "-q"], ["-p", "-q", "-z"], ["-p"]):
        r = _harc(["-d", str(d / "x.harc")] + args + ["-M", str(d / "nothing.txt")])
        assert r.returncode == 1 and "[match] no read of x matches one of the 2 motifs" in r.stdout, r.stdout[-3000:]
        assert _left(d, "x") == before
