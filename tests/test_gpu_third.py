"""Third lines on the GPU.  The yardstick everywhere is the input text itself and the rule restated in Python (tests/third_cases.py).
(i) harc_amd_third_rule_device against that rule on every edge case and on lines of every length at every alignment; (ii) the rule over ingest pieces, whole,
in pieces of a few records and from BGZF, with the additive contract (a bare file and a run without -q leave no member, and the third line reaches no other
file); (iii) a pair; (iv) the assembly under `same` against the Python text; (v) the file call in pieces and as BGZF; (vi) the refusal of an empty id;
(vii) ./harc -c -p -q then -d -p -q on a FASTQ whose third lines repeat the ids gives the input back byte for byte -- whole, gzipped, as a range, as a pair."""
import functools
import gzip
import os
import random
import subprocess
import tarfile

import pytest

from tests import bgzf_util as bu
from tests import idmate_cases as mc
from tests import third_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
K, S, E = 4, 16, 2
TILE = 16384
CASES = tc.cases()


def _dev(b, off=0):
    """the bytes in device memory, `off` bytes behind a 16-byte boundary (the tensor is kept alive by the caller)"""
    import torch
    t = torch.zeros(len(b) + off + 32, dtype=torch.uint8, device="cuda")
    if b:
        t[off:off + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + off


@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        yield h


def _device_rule(ctx, txt, off=0):
    import torch
    t, p = _dev(txt, off)
    torch.cuda.synchronize()                                      # the library works on a stream of its own: its input must be complete
    return ctx.third_rule_device(p, len(txt))


# ------------------------------------------------------------------------------------------------ (i) the rule kernel
@pytest.mark.parametrize("name", sorted(CASES))
def test_rule_device_equals_the_python_rule(ctx, name):
    txt = CASES[name]
    f, n = tc.text_flags(txt)
    for off in (0, 5):
        assert _device_rule(ctx, txt, off) == (tc.EXPECTED[name], n, f), off


@pytest.mark.parametrize("k", range(0, 41))
def test_rule_device_on_lines_of_every_length_at_every_alignment(ctx, k):
    """the text at every residue mod 16; inside it record j's third line starts k + j + 3 bytes behind its id line (tests/third_cases.py: alignment_text)"""
    txt = tc.alignment_text(k)
    f, n = tc.text_flags(txt)
    assert n == 16 and f == (0 if k == 0 else tc.BARE | tc.SAME if k == 1 else tc.SAME)
    for off in range(16):
        assert _device_rule(ctx, txt, off)[1:] == (n, f), off
    # one byte of one third line changed: the first, the second, a middle one, the last -- in a record whose place moves with k
    for byte in sorted({0, 1, k // 2, k - 1} & set(range(k))):
        bad = tc.alignment_text(k, broken=(k % 16, byte))
        assert tc.text_flags(bad) == (0, 16)
        for off in (0, 3, 8, 13):
            assert _device_rule(ctx, bad, off) == ("dropped", 16, 0), (byte, off)


def test_rule_device_more_than_one_wave_and_block(ctx):
    """3000 records are 24 000 lanes, 94 workgroups: one violating record anywhere clears the word, a bare record clears only the same bit's partner"""
    recs = tc.same_file(3000, L=7)
    assert _device_rule(ctx, b"".join(recs), 1) == ("same", 3000, tc.SAME)
    for at in (0, 7, 8, 1499, 2999):
        bad = list(recs)
        bad[at] = tc.record(tc.sra_id(at + 1), b"+" + tc.sra_id(at + 1)[1:-1] + b"Y", L=7)
        assert _device_rule(ctx, b"".join(bad), 1) == ("dropped", 3000, 0), at
    bare = [tc.record(tc.sra_id(i), b"+", L=7) for i in range(3000)]
    assert _device_rule(ctx, b"".join(bare), 9) == ("bare", 3000, tc.BARE)
    bare[2998] = recs[2998]
    assert _device_rule(ctx, b"".join(bare), 9) == ("dropped", 3000, 0)


# ------------------------------------------------------------------------------------------------ (ii) the rule over ingest pieces
N_ING, L_ING = 3001, 100


def _with_thirds(fq, thirds):
    """the FASTQ text with its third lines replaced: thirds = "same", "bare" or {record: line}"""
    ls = fq.split(b"\n")
    n = len(ls) // 4
    for r in range(n):
        if thirds == "same" or (isinstance(thirds, dict) and r not in thirds):
            ls[4 * r + 2] = b"+" + ls[4 * r][1:]
        elif thirds == "bare":
            ls[4 * r + 2] = b"+"
        else:
            ls[4 * r + 2] = thirds[r]
    return b"\n".join(ls)


@functools.lru_cache(maxsize=None)
def _ingest_text(kind):
    fq = bu.fastq_text(N_ING, L_ING, seed=31, n_rate=0.002)
    if kind in ("same", "bare"):
        return _with_thirds(fq, kind)
    at = 3 if kind == "bad_first" else N_ING - 2                  # a record of the first piece only / of the last piece only
    return _with_thirds(fq, {at: b"+r31.%d length=99" % at})


def _files(d):
    return {f: (d / f).read_bytes() for f in sorted(os.listdir(d)) if (d / f).is_file()}


@functools.lru_cache(maxsize=None)
def _ingest_run(kind, route, root, quality=True, order=True):
    """compress_fastq on the text `kind`, ingested by `route` -> the files under output/"""
    import harc_amd
    txt = _ingest_text(kind)
    d = root / ("%s_%s_%d%d" % (kind, route, quality, order))
    os.makedirs(d / "output")
    env = {}
    if route == "bgzf":
        (d / "x.fastq").write_bytes(bu.bgzf(txt, member_text=3000))
        env["HARC_AMD_INGEST_CHUNK"] = str(len(bu.bgzf(txt, member_text=3000)) // 5)
    else:
        (d / "x.fastq").write_bytes(txt)
        if route == "pieces":
            env["HARC_AMD_INGEST_CHUNK"] = "3000"                  # pieces of a few records
        elif route == "streamed":
            env["HARC_AMD_Q_STREAM"] = "1"
            env["HARC_AMD_INGEST_CHUNK"] = "20000"
        elif route == "resident":
            env["HARC_AMD_Q_STREAM"] = "0"
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        harc_amd.compress_fastq(str(d / "x.fastq"), str(d), L_ING, num_thr=E, num_chains=K, num_steps=S, preserve_order=order, preserve_quality=quality)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return _files(d / "output")


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("third")


@pytest.mark.parametrize("route", ["whole", "pieces", "bgzf"])
@pytest.mark.parametrize("kind", ["same", "bad_first", "bad_last"])
def test_the_rule_of_a_job_does_not_depend_on_its_pieces(kind, route, root):
    txt = _ingest_text(kind)
    want = tc.rule(txt)
    assert want == ("same" if kind == "same" else "dropped")
    got = _ingest_run(kind, route, root)
    assert got["read.third"] == b"HARCT1\nthird %s\n" % want.encode()
    assert got["read.third"] == _ingest_run(kind, "whole", root)["read.third"]


@pytest.mark.parametrize("route", ["resident", "streamed"])
def test_the_rule_without_p_on_both_routes_of_q(route, root):
    """-q without -p: the text resident in device memory, or ingested in pieces and streamed again for the side files"""
    assert _ingest_run("same", route, root, order=False)["read.third"] == b"HARCT1\nthird same\n"
    assert _ingest_run("bad_last", route, root, order=False)["read.third"] == b"HARCT1\nthird dropped\n"


@pytest.mark.parametrize("route", ["whole", "pieces", "bgzf"])
def test_a_bare_file_leaves_no_member_and_the_third_line_reaches_nothing_else(route, root):
    """the additive contract: the archive of a bare file has no read.third, and every other file of the run on the `same` text -- the same reads, ids and quality
    values -- equals the bare run's: streams, output.id, output.quality and all"""
    bare = _ingest_run("bare", route, root)
    assert "read.third" not in bare
    same = dict(_ingest_run("same", route, root))
    assert same.pop("read.third") == b"HARCT1\nthird same\n"
    assert sorted(same) == sorted(bare)
    for f in bare:
        assert same[f] == bare[f], f
    ls = _ingest_text("bare").split(b"\n")
    assert bare["output.id"] == b"".join(x + b"\n" for x in ls[0:4 * N_ING:4]) and bare["output.quality"] == b"".join(x + b"\n" for x in ls[3:4 * N_ING:4])


def test_without_q_nothing_is_looked_for_and_nothing_written(root):
    for kind in ("same", "bad_first"):
        got = _ingest_run(kind, "whole", root, quality=False)
        assert "read.third" not in got and "output.id" not in got
        with_q = _ingest_run(kind, "whole", root)
        for f in got:
            assert got[f] == with_q[f], f


# ------------------------------------------------------------------------------------------------ (iii) a pair
def _pair_texts(n, L, style, third="same"):
    ids = {"space": mc.illumina_pairs, "slash": mc.slash_pairs, "same": mc.sra_pairs}[style](n)
    out = []
    for k in range(2):
        rec = bu.fastq_text(n, L, seed=41 + k, n_rate=0.0002).split(b"\n")
        rec[0:4 * n:4] = ids[k]
        out.append(_with_thirds(b"\n".join(rec), third))
    return out


@pytest.mark.parametrize("what", ["both_same", "violation_in_file_2", "both_bare"])
def test_the_rule_of_a_pair_is_over_both_files(what, tmp_path):
    import harc_amd
    n, L = 257, 63
    a, b = _pair_texts(n, L, "space", "bare" if what == "both_bare" else "same")
    if what == "violation_in_file_2":
        ls = b.split(b"\n")
        ls[4 * (n - 1) + 2] = ls[4 * (n - 1) + 2][:-1] + b"Z"
        b = b"\n".join(ls)
    (tmp_path / "a.fastq").write_bytes(a)
    (tmp_path / "b.fastq").write_bytes(b)
    os.makedirs(tmp_path / "output")
    assert harc_amd.compress_fastq_pair(str(tmp_path / "a.fastq"), str(tmp_path / "b.fastq"), str(tmp_path), L, num_thr=E, num_chains=K, num_steps=S, preserve_quality=True) == n
    want = tc.rule(a + b)
    assert want == {"both_same": "same", "violation_in_file_2": "dropped", "both_bare": "bare"}[what] and tc.rule(a) != "dropped"
    got = _files(tmp_path / "output")
    if want == "bare":
        assert "read.third" not in got
    else:
        assert got["read.third"] == b"HARCT1\nthird %s\n" % want.encode()


# ------------------------------------------------------------------------------------------------ (iv) the assembly under `same`
def _text(lines):
    return b"".join(l + b"\n" for l in lines)


def _join_same(ids, reads, quals):
    return b"".join(b"%s\n%s\n+%s\n%s\n" % (i, r, i[1:], q) for i, r, q in zip(ids, reads, quals))


def _lines(rng, n, L, alphabet):
    return [bytes(rng.choice(alphabet) for _ in range(L)) for _ in range(n)]


def _records(seed, n, L, idlens=(1, 2, 15, 16, 17, 27, 49)):
    rng = random.Random(seed)
    ids = [b"@" + bytes(rng.choice(b"abc.:/ 0123456789") for _ in range(rng.choice(idlens) - 1)) for _ in range(n)]
    return ids, _lines(rng, n, L, b"ACGTN"), _lines(rng, n, L, b"#5FHJ+@")


def _assemble_same(h, ids, reads, quals, L, out_off=0):
    """-> the bytes written under the rule same; the 16 bytes either side of the output must stay as they were"""
    import torch
    n = len(ids)
    idtext, dna, qual = _text(ids), _text(reads), _text(quals)
    ti, pi = _dev(idtext, 7)
    td, pd = _dev(dna, 3)
    tq, pq = _dev(qual, 5)
    torch.cuda.synchronize()
    size = h.fastq_assemble_device(pi, len(idtext), pd, pq, n, L, third="same")        # d_out == NULL: validate, size only
    assert size == 2 * len(idtext) + n * (2 * L + 2)
    out = torch.full((size + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    at = 16 + out_off
    torch.cuda.synchronize()
    got = h.fastq_assemble_device(pi, len(idtext), pd, pq, n, L, out.data_ptr() + at, size, third="same")
    torch.cuda.synchronize()
    assert got == size
    host = out.cpu().numpy().tobytes()
    assert host[:at] == b"\xee" * at and host[at + size:] == b"\xee" * (len(host) - at - size), "bytes outside the output were written"
    return host[at:at + size]


@pytest.mark.parametrize("L", [1, 3, 100, 255])
@pytest.mark.parametrize("n", [0, 1, 65, 700])
def test_assembly_under_same_equals_the_python_text(ctx, L, n):
    ids, reads, quals = _records(1000 * L + n, n, L)
    assert _assemble_same(ctx, ids, reads, quals, L, out_off=(L + n) % 16) == _join_same(ids, reads, quals)


def test_assembly_under_same_an_id_of_one_byte(ctx):
    for n in (1, 5):
        ids, reads, quals = [b"@"] * n, [b"ACG"] * n, [b"HHH"] * n
        assert _assemble_same(ctx, ids, reads, quals, 3) == b"@\nACG\n+\nHHH\n" * n


@pytest.mark.parametrize("out_off", range(16))
def test_assembly_under_same_at_every_misalignment_of_the_output(ctx, out_off):
    ids, reads, quals = _records(out_off, 300, 100)
    assert _assemble_same(ctx, ids, reads, quals, 100, out_off=out_off) == _join_same(ids, reads, quals)


def test_assembly_under_same_every_part_of_a_record_straddles_a_tile_edge(ctx):
    """a pad id in front whose length is swept by 1 over 64 values moves every later record by 2 bytes a step, 126 in all, more than the 98 bytes of a record
    of 20 bases with an id of 27: under both parities of the output's misalignment the first tile edge falls on every byte of a record, so its first id, its
    '+', its second id and its quality line each straddle it -- which the sweep itself checks from the Python text"""
    L, n = 20, 400
    ids, reads, quals = _records(9, n, L, idlens=(27,))
    straddled = set()
    for pad in range(1, 65):
        ids[0] = b"@" + b"p" * (pad - 1)
        want = _join_same(ids, reads, quals)
        for out_off in (0, 1):
            assert _assemble_same(ctx, ids, reads, quals, L, out_off=out_off) == want, (pad, out_off)
            edge = TILE - out_off                                 # the output byte at which the second tile begins
            at = 2 * pad + 2 * L + 4                              # where record 1 starts: behind the pad id and its newline, twice, and two lines of L + 1
            r = 1 + (edge - at) // 98
            k = (edge - at) % 98                                  # the byte of record r that is the first of the second tile
            for name, lo, hi in (("id", 0, 26), ("read", 28, 47), ("plus", 48, 50), ("id2", 50, 75), ("quality", 77, 96)):
                if lo < k <= hi:                                  # the part's bytes lo .. hi lie on both sides ('+': the edge falls right in front of or behind it)
                    straddled.add(name)
            assert want[edge - k:edge - k + 28] == ids[r] + b"\n"
    assert straddled == {"id", "read", "plus", "id2", "quality"}


@pytest.mark.parametrize("out_off", [0, 9])
def test_assembly_under_same_an_id_longer_than_a_tile(ctx, out_off):
    L, n = 100, 300
    ids, reads, quals = _records(77, n, L)
    rng = random.Random(3)
    ids[150] = b"@" + bytes(rng.choice(b"abcdefghij0123456789") for _ in range(39999))
    ids[n - 1] = b"@" + bytes(rng.choice(b"klmnopqrst0123456789") for _ in range(39999))
    assert _assemble_same(ctx, ids, reads, quals, L, out_off=out_off) == _join_same(ids, reads, quals)


def test_the_bare_form_is_what_it_was(ctx):
    """the old entry point, the new one with bare and the new one with dropped write the same bytes"""
    import torch
    L, n = 100, 300
    ids, reads, quals = _records(5, n, L, idlens=(0, 1, 16, 27))
    ids = [i[1:] if len(i) == 1 else i for i in ids]                # ids of length 0 are fine under bare
    idtext, dna, qual = _text(ids), _text(reads), _text(quals)
    want = b"".join(b"%s\n%s\n+\n%s\n" % t for t in zip(ids, reads, quals))
    for third in (None, "bare", "dropped"):
        ti, pi = _dev(idtext, 7); td, pd = _dev(dna, 3); tq, pq = _dev(qual, 5)
        out = torch.zeros(len(want) + 32, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        kw = {} if third is None else {"third": third}
        assert ctx.fastq_assemble_device(pi, len(idtext), pd, pq, n, L, out.data_ptr() + 3, len(want), **kw) == len(want)
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes()[3:3 + len(want)] == want, third


# ------------------------------------------------------------------------------------------------ (v) the file call, (vi) the refusal
def _write_three(d, ids, reads, quals):
    (d / "r.dna").write_bytes(_text(reads))
    (d / "r.id").write_bytes(_text(ids))
    (d / "r.quality").write_bytes(_text(quals))
    return str(d / "r.dna"), str(d / "r.id"), str(d / "r.quality")


@pytest.mark.parametrize("piece", [None, "1000", "64"])
def test_file_call_under_same_in_pieces_and_as_bgzf(piece, tmp_path, monkeypatch):
    """pieces of 1000 and of 64 bytes of id text: many pieces, partial lines carried, a piece that has to grow until it holds a line of 300 bytes"""
    import harc_amd
    L, n = 100, 1500
    ids, reads, quals = _records(n, n, L)
    ids[n // 2] = b"@" + b"w" * 299
    want = _join_same(ids, reads, quals)
    assert len(want) > 5 * 65280                                  # several BGZF members, cut inside records
    if piece:
        monkeypatch.setenv("HARC_AMD_FQOUT_PIECE", piece)
        monkeypatch.setenv("HARC_AMD_FEED_SLICE", "256")
    dna, idf, qf = _write_three(tmp_path, ids, reads, quals)
    harc_amd.fastq_assemble(dna, idf, qf, str(tmp_path / "o.fastq"), third="same")
    assert (tmp_path / "o.fastq").read_bytes() == want
    harc_amd.fastq_assemble(dna, idf, qf, str(tmp_path / "o.fastq.gz"), bgzf=True, third="same")
    assert (tmp_path / "o.fastq.gz").read_bytes() == harc_amd.bgzf_deflate_host(want)


@pytest.mark.parametrize("piece", [None, "150"])
@pytest.mark.parametrize("style", ["space", "slash", "same"])
def test_pair_file_call_under_same_carries_each_files_own_ids(style, piece, tmp_path, monkeypatch):
    import harc_amd
    n, L = 300, 63
    a, b = _pair_texts(n, L, style)
    la, lb = a.split(b"\n"), b.split(b"\n")
    (tmp_path / "x.dna").write_bytes(_text(la[1:4 * n:4] + lb[1:4 * n:4]))
    (tmp_path / "x.quality").write_bytes(_text(la[3:4 * n:4] + lb[3:4 * n:4]))
    (tmp_path / "x.id").write_bytes(_text(la[0:4 * n:4]))
    if piece:
        monkeypatch.setenv("HARC_AMD_FQOUT_PIECE", piece)
    o1, o2 = tmp_path / "1.fastq", tmp_path / "2.fastq"
    harc_amd.fastq_assemble_pair(str(tmp_path / "x.dna"), str(tmp_path / "x.id"), str(tmp_path / "x.quality"), str(o1), str(o2), n, style, third="same")
    assert o1.read_bytes() == a and o2.read_bytes() == b


def test_an_empty_id_line_under_same_is_refused_with_its_count(ctx, tmp_path):
    import harc_amd
    import torch
    L, n = 100, 500
    ids, reads, quals = _records(4, n, L)
    for at in (0, 77, 78, n - 1):
        ids[at] = b""
    dna, idf, qf = _write_three(tmp_path, ids, reads, quals)
    out = tmp_path / "o.fastq"
    for bgzf in (False, True):
        out.write_bytes(b"stale")
        with pytest.raises(harc_amd.HarcAmdError) as e:
            harc_amd.fastq_assemble(dna, idf, qf, str(out), bgzf=bgzf, third="same")
        assert e.value.code == EINVAL and "4 id lines are empty" in str(e.value), str(e.value)
        assert not out.exists()
    # the device call refuses the same ids, with and without an output
    idtext = _text(ids)
    ti, pi = _dev(idtext, 7); td, pd = _dev(_text(reads), 3); tq, pq = _dev(_text(quals), 5)
    buf = torch.zeros(2 * len(idtext) + n * (2 * L + 2) + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for o in (None, buf.data_ptr()):
        with pytest.raises(harc_amd.HarcAmdError) as e:
            ctx.fastq_assemble_device(pi, len(idtext), pd, pq, n, L, o, buf.numel() if o else 0, third="same")
        assert e.value.code == EINVAL and "4 id lines are empty" in str(e.value), str(e.value)
    # under bare the same files are records like any other, and a number that names no rule is refused
    harc_amd.fastq_assemble(dna, idf, qf, str(out))
    assert out.read_bytes() == b"".join(b"%s\n%s\n+\n%s\n" % t for t in zip(ids, reads, quals))
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.fastq_assemble(dna, idf, qf, str(out), third=3)
    assert e.value.code == EINVAL and "3 is no rule of the third lines" in str(e.value)


# ------------------------------------------------------------------------------------------------ (vii) ./harc, the round trip
def _harc(args, env=None):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=dict(os.environ, HARC_AMD_STAGE3="none", **(env or {})), stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)


@functools.lru_cache(maxsize=None)
def _sra_fastq(n=2000, L=100):
    """`@SRR1234567.<i> <i> length=100` ids, `+SRR...` third lines, about 2 % of the reads with an N"""
    rec = bu.fastq_text(n, L, seed=61, n_rate=0.0002).split(b"\n")
    assert 20 <= sum(b"N" in r for r in rec[1:4 * n:4]) <= 80
    rec[0:4 * n:4] = [tc.sra_id(i + 1, L) for i in range(n)]
    return _with_thirds(b"\n".join(rec), "same")


@functools.lru_cache(maxsize=None)
def _sra_archive(packed, root):
    d = root / ("cli_%d" % packed)
    d.mkdir()
    (d / "x.fastq").write_bytes(_sra_fastq())
    r = _harc(["-c", str(d / "x.fastq"), "-p", "-q", "-t", "2"] + (["-Q", "-I"] if packed else []))
    assert r.returncode == 0, r.stdout[-3000:]
    return d


def test_harc_c_q_records_the_rule_in_the_archive(root):
    for packed in (False, True):
        with tarfile.open(_sra_archive(packed, root) / "x.harc") as t:
            assert t.extractfile("./read.third").read() == b"HARCT1\nthird same\n"


@pytest.mark.parametrize("packed", [False, True])
def test_harc_roundtrip_of_a_fastq_whose_third_lines_repeat_the_ids(packed, root):
    d = _sra_archive(packed, root)
    fq = _sra_fastq()
    r = _harc(["-d", str(d / "x.harc"), "-p", "-q"])
    assert r.returncode == 0, r.stdout[-3000:]
    got = (d / "x.d.fastq").read_bytes()
    assert len(got) == len(fq), "the restored file holds %d bytes, the input %d" % (len(got), len(fq))
    assert got == fq
    assert not (d / "output").exists()


def test_harc_d_z_and_r_under_same(root):
    d = _sra_archive(True, root)
    fq = _sra_fastq()
    r = _harc(["-d", str(d / "x.harc"), "-p", "-q", "-z"], {"HARC_AMD_FQOUT_PIECE": "7000"})
    assert r.returncode == 0, r.stdout[-3000:]
    assert gzip.decompress((d / "x.d.fastq.gz").read_bytes()) == fq
    r = _harc(["-d", str(d / "x.harc"), "-p", "-q", "-r", "701:1300"])
    assert r.returncode == 0, r.stdout[-3000:]
    assert (d / "x.701-1300.d.fastq").read_bytes() == b"".join(l + b"\n" for l in fq.split(b"\n")[4 * 700:4 * 1300])


@pytest.mark.parametrize("style", ["space", "slash"])
def test_harc_roundtrip_of_a_pair_under_same(style, tmp_path):
    n, L = 500, 100
    a, b = _pair_texts(n, L, style)
    assert tc.rule(a) == tc.rule(b) == "same" and a.split(b"\n")[2] != b.split(b"\n")[2]
    (tmp_path / "s_1.fastq").write_bytes(a)
    (tmp_path / "s_2.fastq").write_bytes(b)
    r = _harc(["-c", str(tmp_path / "s_1.fastq"), "-2", str(tmp_path / "s_2.fastq"), "-p", "-q", "-I", "-t", "2"])
    assert r.returncode == 0, r.stdout[-3000:]
    with tarfile.open(tmp_path / "s_1.harc") as t:
        assert t.extractfile("./read.third").read() == b"HARCT1\nthird same\n"
        assert t.extractfile("./read.pair").read() == b"HARCP1\nrecords %d\nids %s\n" % (n, style.encode())
    r = _harc(["-d", str(tmp_path / "s_1.harc"), "-p", "-q"])
    assert r.returncode == 0, r.stdout[-3000:]
    assert (tmp_path / "s_1.d.1.fastq").read_bytes() == a and (tmp_path / "s_1.d.2.fastq").read_bytes() == b


def test_harc_says_aloud_when_the_third_lines_are_not_kept(tmp_path):
    fq = _with_thirds(bu.fastq_text(300, 100, seed=5), {i: b"+comment %d" % i for i in range(300)})
    (tmp_path / "x.fastq").write_bytes(fq)
    r = _harc(["-c", str(tmp_path / "x.fastq"), "-p", "-q", "-t", "2"])
    assert r.returncode == 0 and "[third] the input's third lines carry text that is not their ids; it is not kept" in r.stdout, r.stdout[-3000:]
    with tarfile.open(tmp_path / "x.harc") as t:
        assert t.extractfile("./read.third").read() == b"HARCT1\nthird dropped\n"
    r = _harc(["-d", str(tmp_path / "x.harc"), "-p", "-q"])
    assert r.returncode == 0 and "[third] the input's third lines carried text other than their ids; it was not kept" in r.stdout, r.stdout[-3000:]
    assert (tmp_path / "x.d.fastq").read_bytes() == _with_thirds(fq, "bare")
    # a bare file: no member, no line, the input back
    (tmp_path / "y.fastq").write_bytes(_with_thirds(fq, "bare"))
    r = _harc(["-c", str(tmp_path / "y.fastq"), "-p", "-q", "-t", "2"])
    assert r.returncode == 0 and "[third]" not in r.stdout, r.stdout[-3000:]
    with tarfile.open(tmp_path / "y.harc") as t:
        assert "./read.third" not in t.getnames()
    r = _harc(["-d", str(tmp_path / "y.harc"), "-p", "-q"])
    assert r.returncode == 0 and "[third]" not in r.stdout and (tmp_path / "y.d.fastq").read_bytes() == _with_thirds(fq, "bare")
