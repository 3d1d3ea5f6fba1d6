"""The range restore on the GPU (./harc -d -r FIRST:LAST; README: "-r and what it promises").  The line select kernels against their host twin at every size,
alignment and place of a newline at which they take another path; the file walk in pieces of a few bytes; the packed side files, of which only the blocks of
the range are unpacked; both decoders over ranges that start and end inside, on and across bins and segments; and ./harc end to end, where every slice is the
slice of the full restore made by the same test."""
import functools
import gzip
import os
import subprocess

import pytest

from tests import bgzf_out_cases as oc
from tests import gen
from tests import idmate_cases as mc
from tests import quality_cases as qc
from tests import range_cases as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFS = (0, 1, 7, 15)


@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        yield h


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("range")


def _on_device(b, lead):
    """b at `lead` bytes behind a 16-byte boundary -> (tensor, device address of b)"""
    import torch
    t = torch.full((lead + len(b) + 64,), 0x0A, dtype=torch.uint8, device="cuda")      # newlines around the text: a byte that is counted by mistake shows
    if b:
        t[lead:lead + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()                                          # the library works on a stream of its own
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + lead


# ------------------------------------------------------------------------------------------------ the kernels
def test_the_kernels_give_what_the_host_twin_gives(ctx):
    import harc_amd
    for name, text in sorted(rc.texts().items()):
        for off in OFFS:
            t, p = _on_device(text, off)
            for k in rc.ks(text):
                want = harc_amd.line_offset_host(text, k)
                assert want == rc.line_offset(text, k)
                assert ctx.line_offset_device(p, len(text), k) == want, (name, off, k)
    assert ctx.line_offset_device(0, 0, 0) == (0, 0) and ctx.line_offset_device(0, 0, 1) == (0, rc.NONE)


def test_the_first_and_the_last_newline_of_a_workgroups_span(ctx):
    """1 MiB of id lines: the spans of the workgroups as harc_amd/csrc/linesel.hip lays them out (rows of 256 chunks of 16 bytes), and for a few of them the
    newlines on both sides of each end"""
    import bisect
    text = rc.id_like()
    n = len(text)
    nls = [i for i, c in enumerate(text) if c == 10]
    nrows = (((n + 30) >> 4) + 255) // 256
    blocks = min(2048, max(1, (nrows + 3) // 4))
    span = -(-nrows // blocks) * 256 * 16
    assert blocks > 8 and span * (blocks - 1) < n
    for off in OFFS:
        t, p = _on_device(text, off)
        asked = set()
        for b in (1, 2, blocks // 2, blocks - 1):
            cut = b * span - off                                   # the first byte of the text that workgroup b owns
            j = bisect.bisect_left(nls, cut)                       # newline j (counted from 0) is the first at or behind it
            asked |= {j - 1, j, j + 1, j + 2}                      # as k: the last two of the span in front, the first two of this one
        for k in sorted(x for x in asked | {len(nls) - 1, len(nls)} if 1 <= x <= len(nls)):      # (the last span may hold a single newline)
            assert ctx.line_offset_device(p, n, k) == (len(nls), nls[k - 1] + 1), (off, k)
        assert ctx.line_offset_device(p, n, len(nls) + 1) == (len(nls), rc.NONE)


# ------------------------------------------------------------------------------------------------ the file walk
def test_the_file_walk_in_pieces_of_a_few_bytes(tmp_path, monkeypatch):
    import harc_amd
    text = rc.lines_of_lengths([3, 0, 12, 7, 40, 0, 5])
    lines = rc.lines_of(text)
    nls = [i for i, c in enumerate(text) if c == 10]
    f = tmp_path / "x.id"
    f.write_bytes(text)
    pieces = (4, 5, 9, 13, 26, 1 << 20)
    # what the pieces are chosen for: one ends on a newline, one a byte behind a newline, one line is longer than a piece
    assert any((i + 1) % 4 == 0 for i in nls) and any((i + 2) % 5 == 0 for i in nls) and max(len(l) for l in lines) > 26
    for piece in pieces:
        monkeypatch.setenv("HARC_AMD_LINESEL_PIECE", str(piece))
        for first, count in ((0, 1), (0, 7), (1, 1), (2, 2), (3, 3), (4, 1), (4, 3), (5, 2), (6, 1), (1, 5)):      # (the last three end in the file's last line)
            b, e = harc_amd.line_range_file(str(f), first, count)
            assert text[b:e] == rc.slice_lines(text, first, count), (piece, first, count)
        assert harc_amd.line_range_file(str(f), 7, 0) == (len(text), len(text)) and harc_amd.line_range_file(str(f), 0, 0) == (0, 0)
        for first, count in ((7, 1), (0, 8), (6, 2), (100, 1)):
            with pytest.raises(harc_amd.HarcAmdError) as err:
                harc_amd.line_range_file(str(f), first, count)
            assert err.value.code == -1 and "lines %d .. %d of" % (first + 1, first + count) in str(err.value) and "holds 7 lines" in str(err.value), str(err.value)
    # a last line without its newline is no line
    (tmp_path / "open.id").write_bytes(text + b"open")
    with pytest.raises(harc_amd.HarcAmdError):
        harc_amd.line_range_file(str(tmp_path / "open.id"), 7, 1)
    (tmp_path / "empty.id").write_bytes(b"")
    with pytest.raises(harc_amd.HarcAmdError):
        harc_amd.line_range_file(str(tmp_path / "empty.id"), 0, 1)


def test_the_file_walk_over_a_file_of_many_pieces(tmp_path, monkeypatch):
    import harc_amd
    text = rc.id_like(300000, seed=4)
    n = text.count(b"\n")
    f = tmp_path / "x.id"
    f.write_bytes(text)
    for piece in (4099, 65536):
        monkeypatch.setenv("HARC_AMD_LINESEL_PIECE", str(piece))
        for first, count in ((0, n), (n - 1, 1), (n // 2, 1), (17, n // 3), (n // 3, n - n // 3)):
            b, e = harc_amd.line_range_file(str(f), first, count)
            assert text[b:e] == rc.slice_lines(text, first, count), (piece, first, count)


# ------------------------------------------------------------------------------------------------ the packed side files
def _ranges(n, rb):
    """(first, count): inside one block, exactly one block, ending on a block's last line, starting on a block's first line, spanning three blocks, the first
    line alone, the last line alone, the whole file"""
    return ((rb + 1, rb // 2), (2 * rb, rb), (rb + 1, rb - 1), (3 * rb, rb // 3), (2 * rb - 1, rb + 2), (0, 1), (n - 1, 1), (0, n))


def _modes(packed, covered=None):
    """the mode byte of every block of a packed side file (of the blocks `covered` alone), by the walk of the 4-byte prefixes"""
    at, out = 32, []
    while at < len(packed):
        out.append(packed[at + 4])
        at += 4 + int.from_bytes(packed[at:at + 4], "little")
    return out if covered is None else [out[b] for b in covered]


@pytest.mark.parametrize("kind, rb", [("quality", 64), ("quality", 4), ("ids", 512), ("ids", 4)])
def test_a_range_of_a_packed_side_file_is_the_slice_of_its_full_unpack(kind, rb, tmp_path, monkeypatch):
    """rb 64 / 512: blocks that are coded; rb 4: every block is stored, the table of a coded block alone is longer than four lines"""
    import harc_amd
    if kind == "quality":
        text, n = qc.markov(1500, 100, seed=7), 1500
        monkeypatch.setenv("HARC_AMD_QPACK_BLOCK", str(rb))
        pack, unpack, unpack_range = harc_amd.qpack_files, harc_amd.qunpack_files, harc_amd.qunpack_range_files
    else:
        text, n = b"".join(l + b"\n" for l in oc.illumina_text(3000).split(b"\n")[0:-1:4]), 3000
        monkeypatch.setenv("HARC_AMD_IDPACK_BLOCK", str(rb))
        pack, unpack, unpack_range = harc_amd.idpack_files, harc_amd.idunpack_files, harc_amd.idunpack_range_files
    assert text.count(b"\n") == n
    src, pk, full, part = tmp_path / "x.txt", tmp_path / "x.packed", tmp_path / "x.full", tmp_path / "x.part"
    src.write_bytes(text)
    pack(str(src), str(pk))
    unpack(str(pk), str(full))
    assert full.read_bytes() == text
    packed = pk.read_bytes()
    assert len(_modes(packed)) == -(-n // rb)
    for piece in (None, "2"):                                      # the blocks of a range in one piece, and in pieces of two blocks
        if piece:
            monkeypatch.setenv("HARC_AMD_QPACK_PIECE" if kind == "quality" else "HARC_AMD_IDPACK_PIECE", piece)
        for k, (first, count) in enumerate(_ranges(n, rb)):
            modes = _modes(packed, range(first // rb, (first + count - 1) // rb + 1))
            # coded blocks are among the covered ones: in every range but the last line alone, whose short block may be stored
            assert (1 in modes or k == 6) if rb > 4 else (set(modes) == {0}), (first, count, modes)
            unpack_range(str(pk), str(part), first, count)
            assert part.read_bytes() == rc.slice_lines(text, first, count), (kind, rb, piece, first, count)
    # blocks outside the range are neither read nor checked: a file that ends inside its last block still gives every line in front of that block
    pk.write_bytes(packed[:-3])
    with pytest.raises(harc_amd.HarcAmdError):
        unpack(str(pk), str(full))
    last = (n - 1) // rb * rb
    unpack_range(str(pk), str(part), last - 7, 7)
    assert part.read_bytes() == rc.slice_lines(text, last - 7, 7)
    with pytest.raises(harc_amd.HarcAmdError) as e:
        unpack_range(str(pk), str(part), last - 7, 8)
    assert "block %d " % ((n - 1) // rb) in str(e.value) and not part.exists(), str(e.value)


# ------------------------------------------------------------------------------------------------ the decoders
N_READS, L, E = 2000, 100, 2


@functools.lru_cache(maxsize=None)
def _reads():
    """2000 reads of 100 bases, reads with N among them (a fiftieth of the errors); the last forty come from a genome of their own, a quarter of their errors N:
    reads that align with nothing, with and without N"""
    a = gen.reads_text(61, N_READS - 40, L, 20000, err=0.01, n_frac=0.02).split()
    b = gen.reads_text(62, 40, L, 4000000, err=0.01, n_frac=0.25).split()
    return tuple(a[:1000] + b[:20] + a[1000:] + b[20:])


@functools.lru_cache(maxsize=None)
def _decoded(root):
    """the archive of _reads() under root/dec (-p, two shards, the library's own K) and its two full decodes"""
    import harc_amd
    d = root / "dec"
    os.makedirs(d / "output")
    reads = _reads()
    (d / "in.fastq").write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * L) for i, r in enumerate(reads)))
    harc_amd.compress_fastq(str(d / "in.fastq"), str(d), L, num_thr=E, num_chains=0, preserve_order=True)
    harc_amd.pack_order(str(d), L)
    full = {}
    for keep in (False, True):
        harc_amd.decoder(str(d), E, preserve_order=keep)
        full[keep] = (d / "output" / "output.dna").read_bytes()
    assert full[True] == b"".join(r + b"\n" for r in reads) and sorted(full[False].split()) == sorted(reads)
    return d, full


def _size(d, name):
    return os.path.getsize(d / "output" / name)


def test_ranges_of_the_decoder_without_p(root):
    import harc_amd
    d, full = _decoded(root)
    text = full[False]
    lines = rc.lines_of(text)
    # the segments of the output, read from the full decode: each shard's lines without N, the singletons, each shard's lines with N, input_N.dna
    shard = [_size(d, "read_pos.txt.%d" % e) for e in range(E)]
    ns = (4 * _size(d, "read_singleton.txt") + _size(d, "read_singleton.txt.tail")) // L
    nu = _size(d, "input_N.dna") // (L + 1)
    clean = next(i for i, l in enumerate(lines) if b"N" in l)       # where the lines with N begin
    assert all(b"N" in l for l in lines[clean:]) and sum(shard) + ns + nu == N_READS
    aligned = clean - ns                                            # lines without N of all shards
    with_n = sum(shard) - aligned                                   # lines with N of all shards
    assert ns >= 3 and nu >= 3 and with_n >= 3 and shard[0] - with_n > 200 and shard[1] > with_n
    ranges = {
        "inside shard 0's lines": (100, 57),                        # (shard 0 has at least shard[0] - with_n lines without N)
        "the first line": (0, 1),
        "from shard 0's lines into shard 1's": (shard[0] - with_n - 5, with_n + 10),
        "from shard lines into the singletons": (aligned - 4, 6),
        "over all singletons into the lines with N": (aligned - 2, ns + 4),
        "from the singletons into the lines with N": (clean - 2, 4),
        "from the lines with N into input_N.dna": (N_READS - nu - 2, 4),
        "the last line": (N_READS - 1, 1),
        "everything": (0, N_READS),
    }
    assert ranges["from shard lines into the singletons"][0] + 6 <= clean and N_READS - nu - 2 >= clean
    for what, (first, count) in ranges.items():
        harc_amd.decoder(str(d), E, ranges=[(first, count)])
        assert (d / "output" / "output.dna").read_bytes() == rc.slice_lines(text, first, count), what
    a, b = ranges["from shard lines into the singletons"], ranges["from the lines with N into input_N.dna"]
    for two in ((a, b), (b, a), ((0, 10), (5, 10))):                # in the order they are given, and overlapping
        harc_amd.decoder(str(d), E, ranges=list(two))
        assert (d / "output" / "output.dna").read_bytes() == rc.slice_lines(text, *two[0]) + rc.slice_lines(text, *two[1]), two
    for first, count in ((N_READS, 1), (N_READS - 1, 2), (0, N_READS + 1), (5, 0)):
        with pytest.raises(harc_amd.HarcAmdError) as e:
            harc_amd.decoder(str(d), E, ranges=[(first, count)])
        assert e.value.code == -1 and "the archive holds %d" % N_READS in str(e.value), str(e.value)
    harc_amd.decoder(str(d), E)                                     # ... and without a range everything is what it was
    assert (d / "output" / "output.dna").read_bytes() == text


@pytest.mark.parametrize("bin_reads", [None, 64])
def test_ranges_of_the_decoder_with_p(root, bin_reads, monkeypatch):
    """bins of 64 lines: ranges inside a bin, of exactly one, ending where one ends, and across three; a bin starts where its range starts"""
    import harc_amd
    d, full = _decoded(root)
    text = full[True]
    if bin_reads:
        monkeypatch.setenv("HARC_AMD_BIN_READS", str(bin_reads))
    for first, count in ((10, 20), (0, 64), (64, 64), (37, 27), (100, 133), (0, 1), (N_READS - 1, 1), (N_READS - 70, 70), (1000, 20), (0, N_READS)):
        harc_amd.decoder(str(d), E, preserve_order=True, ranges=[(first, count)])
        assert (d / "output" / "output.dna").read_bytes() == rc.slice_lines(text, first, count), (first, count)
    for two in (((10, 100), (1010, 100)), ((1010, 100), (10, 100)), ((0, 65), (64, 2))):
        harc_amd.decoder(str(d), E, preserve_order=True, ranges=list(two))
        assert (d / "output" / "output.dna").read_bytes() == rc.slice_lines(text, *two[0]) + rc.slice_lines(text, *two[1]), two
    for first, count in ((N_READS, 1), (N_READS - 1, 2), (7, 0)):
        with pytest.raises(harc_amd.HarcAmdError) as e:
            harc_amd.decoder(str(d), E, preserve_order=True, ranges=[(first, count)])
        assert e.value.code == -1 and "the archive holds %d" % N_READS in str(e.value), str(e.value)
    harc_amd.decoder(str(d), E, preserve_order=True)
    assert (d / "output" / "output.dna").read_bytes() == text


# ------------------------------------------------------------------------------------------------ the command line
def _harc(args, env=None):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=dict(os.environ, HARC_AMD_STAGE3="none", **(env or {})), stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)


def _fastq(n, seed, ids=None, n_frac=0.02):
    reads = gen.reads_text(seed, n, L, 15000, err=0.01, n_frac=n_frac).split()
    quals = qc.markov(n, L, seed=seed).split()
    ids = ids or oc.illumina_text(n).split(b"\n")[0:-1:4]
    return b"".join(b"%s\n%s\n+\n%s\n" % t for t in zip(ids, reads, quals))


def _left(d, stem):
    """what a restore has written next to the archive"""
    return sorted(f for f in os.listdir(d) if f.startswith(stem + ".") and (".d." in f or f.endswith(".dna.d"))) + (["output"] if (d / "output").exists() else [])


@functools.lru_cache(maxsize=None)
def _archive(kind, root):
    """./harc -c, once per kind of archive -> (its directory, the FASTQ text or the two texts of a pair).  packed: -p -q -Q -I, six quality blocks and three id
    blocks; stored: -q -V without -p, text side files, reads without N so that the ids sit on their records (README: the .id file of a run without -p);
    pair_space / pair_none: -c R1 -2 R2 -p -q -I with ids that give the rule space, and with the second file's ids in another order"""
    d = root / kind
    d.mkdir()
    if kind == "packed":
        fq = _fastq(1500, 71)
        (d / "x.fastq").write_bytes(fq)
        r = _harc(["-c", str(d / "x.fastq"), "-p", "-q", "-Q", "-I", "-t", "2"], {"HARC_AMD_QPACK_BLOCK": "256", "HARC_AMD_IDPACK_BLOCK": "512"})
        assert r.returncode == 0 and (d / "x.quality.hq").exists() and (d / "x.id.hi").exists() and not (d / "x.id").exists(), r.stdout[-3000:]
    elif kind == "stored":
        fq = _fastq(1200, 73, n_frac=0.0)
        (d / "x.fastq").write_bytes(fq)
        r = _harc(["-c", str(d / "x.fastq"), "-q", "-V", "-t", "2"])
        assert r.returncode == 0 and (d / "x.quality").exists() and (d / "x.id").exists(), r.stdout[-3000:]
    else:
        a_ids, b_ids = mc.illumina_pairs(600)
        if kind == "pair_none":
            b_ids = tuple(reversed(b_ids))
        fq = _fastq(600, 75, list(a_ids)), _fastq(600, 76, list(b_ids))
        (d / "x.fastq").write_bytes(fq[0])
        (d / "x_2.fastq").write_bytes(fq[1])
        r = _harc(["-c", str(d / "x.fastq"), "-2", str(d / "x_2.fastq"), "-p", "-q", "-I", "-t", "2"], {"HARC_AMD_IDPACK_BLOCK": "128"})
        assert r.returncode == 0 and (d / "x.id.hi").exists() and (d / "x.quality").exists(), r.stdout[-3000:]
        assert ("ids %s" % kind[5:]) in subprocess.run(["tar", "-xOf", str(d / "x.harc"), "./read.pair"], stdout=subprocess.PIPE, text=True).stdout
    return d, fq


def test_harc_restores_a_range_of_a_packed_archive_plain_and_gzipped(root):
    import harc_amd
    d, fq = _archive("packed", root)
    r = _harc(["-d", str(d / "x.harc"), "-p", "-q"])
    assert r.returncode == 0 and (d / "x.d.fastq").read_bytes() == fq, r.stdout[-3000:]
    full = (d / "x.d.fastq").read_bytes()
    want = rc.slice_records(full, 700, 600)
    assert want.count(b"\n") == 2400
    r = _harc(["-d", str(d / "x.harc"), "-p", "-q", "-r", "701:1300"])
    assert r.returncode == 0, r.stdout[-3000:]
    assert (d / "x.701-1300.d.fastq").read_bytes() == want
    # only the blocks of the range were unpacked
    assert "[qunpack] lines 701 .. 1300 of 1500: blocks 2 .. 5 of 6" in r.stdout and "[idunpack] lines 701 .. 1300 of 1500: blocks 1 .. 2 of 3" in r.stdout, r.stdout[-3000:]
    r = _harc(["-d", str(d / "x.harc"), "-p", "-q", "-z", "-r", "701:1300"])
    assert r.returncode == 0, r.stdout[-3000:]
    gz = (d / "x.701-1300.d.fastq.gz").read_bytes()
    assert gzip.decompress(gz) == want and gz == harc_amd.bgzf_deflate_host(want)
    assert (d / "x.d.fastq").read_bytes() == full and not (d / "output").exists()      # a slice never replaces a full restore


def test_harc_restores_a_range_of_the_reads_alone_and_refuses_a_last_beyond_them(root):
    d, fq = _archive("packed", root)
    r = _harc(["-d", str(d / "x.harc"), "-p"])
    assert r.returncode == 0, r.stdout[-3000:]
    full = (d / "x.dna.d").read_bytes()
    assert full == b"".join(l + b"\n" for l in fq.split(b"\n")[1::4])
    r = _harc(["-d", str(d / "x.harc"), "-p", "-r", "701:1300"])
    assert r.returncode == 0 and (d / "x.701-1300.dna.d").read_bytes() == rc.slice_lines(full, 700, 600), r.stdout[-3000:]
    # LAST = N + 1: refused by the stage program, naming both, and nothing is left
    before = _left(d, "x")
    for args in (["-p", "-q"], []):
        r = _harc(["-d", str(d / "x.harc")] + args + ["-r", "1400:1501"])
        assert r.returncode == 1 and "1501" in r.stdout and "holds 1500" in r.stdout, r.stdout[-3000:]
        assert _left(d, "x") == before


@pytest.mark.parametrize("first, last", [(1, 1), (1200, 1200), (600, 699)])
def test_harc_restores_records_in_stored_order_and_says_what_is_not_checked(first, last, root):
    d, fq = _archive("stored", root)
    r = _harc(["-d", str(d / "x.harc"), "-q"])
    assert r.returncode == 0 and "[check] reads ok" in r.stdout, r.stdout[-3000:]
    full = (d / "x.d.fastq").read_bytes()
    assert sorted(rc.lines_of(full)[1::4]) == sorted(l + b"\n" for l in fq.split(b"\n")[1::4]) and full != fq
    r = _harc(["-d", str(d / "x.harc"), "-q", "-r", "%d:%d" % (first, last)], {"HARC_AMD_LINESEL_PIECE": "5000"})
    assert r.returncode == 0, r.stdout[-3000:]
    assert "[check] not checked: -r restores a part of the archive (./harc -v checks all of it)" in r.stdout and "reads ok" not in r.stdout
    assert (d / ("x.%d-%d.d.fastq" % (first, last))).read_bytes() == rc.slice_records(full, first - 1, last - first + 1)


def test_harc_refuses_a_last_beyond_the_records_in_stored_order(root):
    d, fq = _archive("stored", root)
    before = _left(d, "x")
    r = _harc(["-d", str(d / "x.harc"), "-q", "-r", "1200:1201"])
    assert r.returncode == 1 and "1201" in r.stdout and "holds 1200" in r.stdout, r.stdout[-3000:]
    assert _left(d, "x") == before and not (d / "output").exists()


@pytest.mark.parametrize("style", ["space", "none"])
def test_harc_restores_a_range_of_each_file_of_a_pair(style, root):
    d, (a, b) = _archive("pair_" + style, root)
    r = _harc(["-d", str(d / "x.harc"), "-p", "-q"])
    assert r.returncode == 0, r.stdout[-3000:]
    full = (d / "x.d.1.fastq").read_bytes(), (d / "x.d.2.fastq").read_bytes()
    assert full == (a, b)
    r = _harc(["-d", str(d / "x.harc"), "-p", "-q", "-r", "10:500"])
    assert r.returncode == 0, r.stdout[-3000:]
    assert (d / "x.10-500.d.1.fastq").read_bytes() == rc.slice_records(full[0], 9, 491)
    assert (d / "x.10-500.d.2.fastq").read_bytes() == rc.slice_records(full[1], 9, 491)      # mates stay together
    assert r.stdout.count("[idunpack] lines") == (2 if style == "none" else 1), r.stdout[-3000:]


def test_harc_refuses_a_last_beyond_the_records_of_a_pair(root):
    d, _ = _archive("pair_space", root)
    before = _left(d, "x")
    r = _harc(["-d", str(d / "x.harc"), "-p", "-q", "-r", "600:601"])
    assert r.returncode == 1 and "LAST is 601, each file of the pair holds 600 records" in r.stdout, r.stdout[-3000:]
    assert _left(d, "x") == before
