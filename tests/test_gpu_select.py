"""Selection by name on the GPU (./harc -d -q -L NAMES; README: "-L and what it promises").  The device calls against the plain-Python restatement of
tests/select_cases.py on every case, with both texts at device addresses misaligned by 0, 1 and 15 bytes among bytes that would change a name if they were
read, under 64, 8 and 1 bits of the hash; the gathers into a misaligned output between guard bytes; a larger list; the file call in pieces of a few bytes and
lines, with the pair layouts and its refusals; and ./harc end to end, where every selection is the restatement's filter of the input."""
import functools
import gzip
import os
import subprocess

import pytest

from tests import bgzf_out_cases as oc
from tests import gen
from tests import idmate_cases as mc
from tests import quality_cases as qc
from tests import select_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sc.cases()
LEADS = (0, 1, 15)
N_IDS = 3001
L = 100


@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        yield h


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("select")


def _on_device(b, lead, fill=0x41, tail=64):
    """b at `lead` bytes behind the start of an allocation -> (tensor, device address of b); the bytes around it are 'A': a name that reads them is another name"""
    import torch
    t = torch.full((lead + len(b) + tail,), fill, dtype=torch.uint8, device="cuda")
    if b:
        t[lead:lead + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()                                          # the library works on a stream of its own
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + lead


def _flags_device(ctx, names, ids, lead_n, lead_i):
    tn, pn = _on_device(names, lead_n)
    ti, pi = _on_device(ids, lead_i)
    n = len(sc.lines(ids))
    tf, pf = _on_device(b"\x55" * n, 3, fill=0x77)
    got = ctx.select_flags_device(pn if names else 0, len(names), pi if ids else 0, len(ids), pf)
    raw = bytes(tf.cpu().numpy().tobytes())
    assert raw[:3] == b"\x77" * 3 and raw[3 + n:] == b"\x77" * 64, "bytes around the flags were written"
    return raw[3:3 + n], got


# ------------------------------------------------------------------------------------------------ the device calls
@pytest.mark.parametrize("bits", [64, 8, 1])
@pytest.mark.parametrize("lead_n, lead_i", [(0, 0), (1, 15), (15, 1)])
def test_select_flags_device_equals_the_restatement(ctx, monkeypatch, bits, lead_n, lead_i):
    if bits != 64:
        monkeypatch.setenv("HARC_AMD_SELECT_HASH_BITS", str(bits))
    for name in sorted(CASES):
        names, ids = CASES[name]
        flags, (n_lines, n_names, n_found) = _flags_device(ctx, names, ids, lead_n, lead_i)
        assert flags == sc.flags(names, ids), (name, bits, lead_n, lead_i)
        assert (n_lines, n_names, n_found) == (len(sc.lines(ids)),) + sc.counts(names, ids), (name, bits)


def test_select_flags_device_is_what_the_host_twin_gives(ctx):
    import harc_amd
    for name in sorted(CASES):
        names, ids = CASES[name]
        flags, (n_lines, n_names, n_found) = _flags_device(ctx, names, ids, 7, 9)
        assert (flags, n_names, n_found) == harc_amd.select_flags_host(names, ids), name


def test_select_flags_device_on_empty_texts(ctx):
    tn, pn = _on_device(b"a\n", 0)
    assert ctx.select_flags_device(pn, 2, 0, 0, 0) == (0, 1, 0)
    flags, got = _flags_device(ctx, b"", b"@a\n@b\n", 0, 0)
    assert flags == b"\0\0" and got == (2, 0, 0)


@pytest.mark.parametrize("lead_out", [0, 1, 15])
def test_lines_gather_device_equals_the_restatement_and_touches_nothing_else(ctx, lead_out):
    for name, (text, f, stride) in sorted(sc.gather_cases().items()):
        want = sc.gather(text, f, stride)
        tt, pt = _on_device(text, (lead_out + 5) % 16)
        tf, pf = _on_device(f, 2)
        to, po = _on_device(b"\x55" * len(want), lead_out, fill=0x77)
        n = ctx.lines_gather_device(pt, len(text), stride, pf, len(f), po, len(want))
        raw = bytes(to.cpu().numpy().tobytes())
        assert n == len(want) and raw == b"\x77" * lead_out + want + b"\x77" * 64, (name, lead_out)


def test_lines_gather_device_takes_any_flag_byte_that_is_not_zero_and_refuses_too_little_room(ctx):
    import harc_amd
    text = b"ab\ncd\nef\n"
    tt, pt = _on_device(text, 1)
    tf, pf = _on_device(bytes([7, 0, 255]), 0)
    to, po = _on_device(b"\x55" * 6, 5, fill=0x77)
    assert ctx.lines_gather_device(pt, len(text), 3, pf, 3, po, 6) == 6
    assert bytes(to.cpu().numpy().tobytes())[5:11] == b"ab\nef\n"
    assert ctx.lines_gather_device(pt, len(text), 0, pf, 3, po, 6) == 6
    for stride in (0, 3):
        with pytest.raises(harc_amd.HarcAmdError, match="take 6 bytes, the output has room for 5"):
            ctx.lines_gather_device(pt, len(text), stride, pf, 3, po, 5)
    with pytest.raises(harc_amd.HarcAmdError, match="holds 3 lines, the flags are those of 2"):
        ctx.lines_gather_device(pt, len(text), 0, pf, 2, po, 6)


# ------------------------------------------------------------------------------------------------ a larger list
@functools.lru_cache(maxsize=None)
def _larger():
    ids = oc.illumina_text(N_IDS).split(b"\n")[0:-1:4]
    assert len(ids) == N_IDS
    picked = [ids[(i * 6007) % N_IDS] for i in range(500)]
    absent = [b"SRR870667.%d" % (N_IDS + 1 + i) for i in range(20)]
    listed = []
    for k, l in enumerate(picked):
        listed.append(sc.key(l) if k % 2 else l)                     # a bare name, or the id line as it stands
        if k % 25 == 0:
            listed.append(absent[k // 25])
    return b"".join(l + b"\n" for l in ids), b"".join(l + b"\n" for l in listed), absent


def test_a_larger_list_over_more_than_one_workgroup(ctx, tmp_path):
    import harc_amd
    ids, names, absent = _larger()
    want = sc.flags(names, ids)
    assert sum(want) == 500 and sc.counts(names, ids) == (520, 500)
    for lead in (0, 9):
        flags, got = _flags_device(ctx, names, ids, lead, 16 - lead)
        assert flags == want and got == (N_IDS, 520, 500)
    # which names are reported missing: the file call, over reads of 4
    for name, text in (("n", names), ("i", ids), ("d", b"ACGT\n" * N_IDS), ("q", b"IIII\n" * N_IDS)):
        (tmp_path / name).write_bytes(text)
    p = [str(tmp_path / x) for x in ("n", "i", "d", "q", "oi", "od", "oq")]
    st = harc_amd.select_files(*p)
    assert st[:4] == (520, 500, 500, N_IDS) and st[4] == absent[:10] == sc.missing(names, ids)
    assert (tmp_path / "oi").read_bytes() == sc.gather(ids, want) and (tmp_path / "od").read_bytes() == b"ACGT\n" * 500


def test_offsets_past_2_31_bytes(ctx):
    """an id text of more than 2^31 bytes, made on the device: the first line, the first line that starts past byte 2^31 and the last one are listed; then the
    same three lines gathered by the stride"""
    import torch
    head, tail = b"@SRR870667.", b" HWI-ST1234:100:C0ABCACXX:3:1101:12345:123456 length=100\n"
    width = len(head) + 8 + len(tail)
    n = (2 ** 31 + 2 ** 27) // width
    t = torch.frombuffer(bytearray(head + b"00000000" + tail), dtype=torch.uint8).to("cuda").repeat(n, 1)
    idx = torch.arange(n, device="cuda", dtype=torch.int64)
    for k in range(8):
        t[:, len(head) + k] = (48 + (idx // 10 ** (7 - k)) % 10).to(torch.uint8)
    del idx
    t = t.reshape(-1)
    past = 2 ** 31 // width + 1
    assert past * width > 2 ** 31 and n * width < 2 ** 32
    picked = [0, past, n - 1]
    names = b"".join(b"SRR870667.%08d\n" % i for i in picked) + b"SRR870667.%08d\n" % n
    tn, pn = _on_device(names, 5)
    flags = torch.full((n + 64,), 0x77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.select_flags_device(pn, len(names), t.data_ptr(), n * width, flags.data_ptr()) == (n, 4, 3)
    assert torch.nonzero(flags[:n])[:, 0].tolist() == picked and int(flags[n:].min()) == 0x77
    out = torch.full((3 * width + 64,), 0x77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.lines_gather_device(t.data_ptr(), n * width, width, flags.data_ptr(), n, out.data_ptr() + 3, 3 * width) == 3 * width
    got = bytes(out.cpu().numpy().tobytes())
    assert got == b"\x77" * 3 + b"".join(head + b"%08d" % i + tail for i in picked) + b"\x77" * 61


# ------------------------------------------------------------------------------------------------ the file call
def _nm(i):
    return b"r%d%s" % (i, b"x" * (i * 5 % 23))


def _job(n, pair=None):
    """ids of n records whose lines differ in length, reads and quality values of 6 that tell their record; pair: 'space' or 'none' -> the job of 2 n records"""
    ids = [b"@%s len=%d" % (_nm(i), i) for i in range(n)]
    total = 2 * n if pair else n
    dna = b"".join(b"%05dA\n" % i for i in range(total))
    quality = b"".join(b"%05dI\n" % i for i in range(total))
    if pair == "none":
        ids = ids + [b"@m%d/2 mate" % i for i in range(n)]
    return b"".join(l + b"\n" for l in ids), dna, quality


def _select_files(tmp_path, names, ids, dna, quality, **kw):
    import harc_amd
    for name, text in (("n", names), ("i", ids), ("d", dna), ("q", quality)):
        (tmp_path / name).write_bytes(text)
    for name in ("oi", "od", "oq"):
        if (tmp_path / name).exists():
            os.remove(tmp_path / name)
    p = [str(tmp_path / x) for x in ("n", "i", "d", "q", "oi", "od", "oq")]
    st = harc_amd.select_files(*p, **kw)
    return st, tuple((tmp_path / x).read_bytes() for x in ("oi", "od", "oq"))


@pytest.mark.parametrize("piece, lines", [("7", "3"), ("333", "3"), ("333", None), (None, None)])
def test_select_files_in_pieces(tmp_path, monkeypatch, piece, lines):
    if piece:
        monkeypatch.setenv("HARC_AMD_SELECT_PIECE", piece)
    if lines:
        monkeypatch.setenv("HARC_AMD_SELECT_LINES", lines)
    n = 41
    ids, dna, quality = _job(n)
    starts = [0]
    for l in sc.lines(ids):
        starts.append(starts[-1] + len(l) + 1)
    # selected: the first and the last record, one whose line ends at byte 333's piece boundary or crosses it, the line in front of it and the one behind it
    cross = max(i for i in range(n) if starts[i] < 333)
    assert starts[cross] < 333 < starts[cross + 1]
    for sel in ([0, n - 1, cross - 1, cross, cross + 1], [cross], list(range(n)), [2, 3, 4, 5, 6, 7]):
        names = b"".join(_nm(i) + b"\n" for i in sel) + b"nobody\n"
        want = sc.flags(names, ids)
        assert [i for i in range(n) if want[i]] == sorted(sel)
        st, (oi, od, oq) = _select_files(tmp_path, names, ids, dna, quality)
        assert st == (len(sel) + 1, len(sel), len(sel), n, [b"nobody"]), (piece, lines, sel)
        assert oi == sc.gather(ids, want) and od == sc.gather(dna, want, 7) and oq == sc.gather(quality, want, 7), (piece, lines, sel)


@pytest.mark.parametrize("piece, lines", [("7", "3"), (None, None)])
def test_select_files_on_the_layouts_of_a_pair(tmp_path, monkeypatch, piece, lines):
    if piece:
        monkeypatch.setenv("HARC_AMD_SELECT_PIECE", piece)
        monkeypatch.setenv("HARC_AMD_SELECT_LINES", lines)
    n = 17
    # a rule: X.id holds file 1's ids alone, record i of both files goes with id line i
    ids, dna, quality = _job(n, "space")
    names = _nm(3) + b"\n" + _nm(16) + b"/2\n" + _nm(0) + b"\n"
    f = sc.flags(names, ids)
    assert [i for i in range(n) if f[i]] == [0, 3, 16]
    st, (oi, od, oq) = _select_files(tmp_path, names, ids, dna, quality, pair_records=n, pair_rule="space")
    assert st == (3, 3, 3, n, [])
    assert oi == sc.gather(ids, f) and od == sc.gather(dna, f + f, 7) and oq == sc.gather(quality, f + f, 7)
    # none: X.id holds 2 n lines, pair i is selected when line i or line n + i is listed
    ids, dna, quality = _job(n, "none")
    names = _nm(3) + b"\nm5\nm16/1\nm3\nabsent\n"
    half = sc.flags(names, ids)
    assert [i for i in range(2 * n) if half[i]] == [3, n + 3, n + 5, n + 16]
    f = bytes(half[i] | half[n + i] for i in range(n))
    st, (oi, od, oq) = _select_files(tmp_path, names, ids, dna, quality, pair_records=n, pair_rule="none")
    assert st == (5, 4, 3, n, [b"absent"])
    assert oi == sc.gather(ids, f + f) and od == sc.gather(dna, f + f, 7) and oq == sc.gather(quality, f + f, 7)


def test_select_files_of_nothing_gives_three_empty_files(tmp_path):
    ids, dna, quality = _job(9)
    st, outs = _select_files(tmp_path, b"nobody\n", ids, dna, quality)
    assert st == (1, 0, 0, 9, [b"nobody"]) and outs == (b"", b"", b"")


def test_select_files_refuses_what_does_not_fit_and_leaves_no_output(tmp_path):
    import harc_amd
    ids, dna, quality = _job(9)
    none_ids, dna2, quality2 = _job(9, "none")
    big = tmp_path / "big"
    with open(big, "wb") as f:
        f.truncate(2 ** 30 + 1)
    cases = [
        (dict(ids=ids + b"@one more\n"), {}, "holds 10 lines, .* 9 reads"),
        (dict(ids=ids[:-1].rsplit(b"\n", 1)[0] + b"\n"), {}, "holds 8 lines, .* 9 reads"),
        (dict(quality=quality + b"00009I\n"), {}, "holds 70 bytes, .* 63"),
        (dict(ids=ids, dna=dna2, quality=quality2), dict(pair_records=9, pair_rule="none"), "holds 9 lines, a pair of 9 records under the rule none has 18"),
        (dict(ids=none_ids, dna=dna2, quality=quality2), dict(pair_records=9, pair_rule="slash"), "holds 18 lines, a pair of 9 records under the rule slash has 9"),
        (dict(ids=ids, dna=dna2, quality=quality2), dict(pair_records=8, pair_rule="slash"), "a pair of 8 records is wanted, .* holds 18 reads"),
        (dict(names=b"\n@\n \n"), {}, "no line of the list .* has a name"),
        (dict(names=b""), {}, "is empty"),
    ]
    for texts, kw, words in cases:
        t = dict(names=_nm(1) + b"\n", ids=ids, dna=dna, quality=quality)
        t.update(texts)
        with pytest.raises(harc_amd.HarcAmdError, match=words) as e:
            _select_files(tmp_path, t["names"], t["ids"], t["dna"], t["quality"], **kw)
        assert e.value.code == -1, str(e.value)
        assert not any((tmp_path / x).exists() for x in ("oi", "od", "oq")), words
    with pytest.raises(harc_amd.HarcAmdError, match="1073741825 bytes, more than the 1073741824"):
        harc_amd.select_files(str(big), *[str(tmp_path / x) for x in ("i", "d", "q", "oi", "od", "oq")])
    assert not any((tmp_path / x).exists() for x in ("oi", "od", "oq"))


# ------------------------------------------------------------------------------------------------ the command line
def _harc(args, env=None):
    e = dict(os.environ, HARC_AMD_STAGE3="none")
    e.update(env or {})
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _fastq(n, seed, ids=None, n_frac=0.02, third=False):
    reads = gen.reads_text(seed, n, L, 15000, err=0.01, n_frac=n_frac).split()
    quals = qc.markov(n, L, seed=seed).split()
    ids = ids or oc.illumina_text(n).split(b"\n")[0:-1:4]
    return b"".join(b"%s\n%s\n+%s\n%s\n" % (i, r, i[1:] if third else b"", q) for i, r, q in zip(ids, reads, quals))


def _left(d, stem):
    """what a restore has written next to the archive"""
    return sorted(f for f in os.listdir(d) if f.startswith(stem + ".") and (".d." in f or f.endswith(".dna.d"))) + (["output"] if (d / "output").exists() else [])


def _pair_ids(style, n):
    if style == "slash":
        return mc.slash_pairs(n)
    a, b = mc.illumina_pairs(n)
    if style == "none":                                               # the mates carry names of their own: no rule makes file 2's ids from file 1's
        b = tuple(x.split(b" ")[0] + b"_m/2 mate" for x in b)
    return a, b


@functools.lru_cache(maxsize=None)
def _archive(kind, root):
    """./harc -c, once per kind of archive -> (its directory, the FASTQ text or the two texts of a pair)"""
    d = root / kind
    d.mkdir()
    if kind in ("plain", "packed", "third", "stored"):
        n = 1200 if kind in ("plain", "packed") else 400
        fq = _fastq(n, 81, n_frac=0.0 if kind == "stored" else 0.02, third=kind == "third")
        (d / "x.fastq").write_bytes(fq)
        flags = {"plain": ["-p", "-q"], "packed": ["-p", "-q", "-Q", "-I", "-S", "-V"], "third": ["-p", "-q"], "stored": ["-q"]}[kind]
        env = {"HARC_AMD_QPACK_BLOCK": "256", "HARC_AMD_IDPACK_BLOCK": "512"}
        if kind == "packed":
            env["HARC_AMD_STAGE3"] = "auto"                           # (-S is the packer)
        r = _harc(["-c", str(d / "x.fastq")] + flags + ["-t", "2"], env)
        assert r.returncode == 0 and (d / "x.harc").exists(), r.stdout[-3000:]
    else:
        a_ids, b_ids = _pair_ids(kind[5:], 400)
        fq = _fastq(400, 85, list(a_ids)), _fastq(400, 86, list(b_ids))
        (d / "x.fastq").write_bytes(fq[0])
        (d / "x_2.fastq").write_bytes(fq[1])
        r = _harc(["-c", str(d / "x.fastq"), "-2", str(d / "x_2.fastq"), "-p", "-q", "-t", "2"])
        assert r.returncode == 0 and (d / "x.id").exists(), r.stdout[-3000:]
        assert ("ids %s" % kind[5:]) in subprocess.run(["tar", "-xOf", str(d / "x.harc"), "./read.pair"], stdout=subprocess.PIPE, text=True).stdout
    return d, fq


def _list_of(fq, every, extra=(b"nobody/1", b"", b"@")):
    """every `every`-th name of a FASTQ text, alternately bare and as the id line stands, in another order than the file's, with a duplicate and lines that name
    nothing in the file"""
    ids = fq.split(b"\n")[0:-1:4][::every]
    lines = [sc.key(l) if k % 2 else l for k, l in enumerate(ids)]
    return b"".join(l + b"\n" for l in list(reversed(lines)) + [lines[0]] + list(extra))


@pytest.mark.parametrize("kind", ["plain", "packed", "third"])
def test_harc_selects_by_name_plain_and_gzipped(kind, root):
    import harc_amd
    d, fq = _archive(kind, root)
    names = _list_of(fq, 37)
    (d / "names.txt").write_bytes(names)
    want = sc.select_fastq(fq, names)
    k = want.count(b"\n") // 4
    n = fq.count(b"\n") // 4
    assert 1 < k < n / 10
    r = _harc(["-d", str(d / "x.harc"), "-p", "-q", "-L", str(d / "names.txt")], {"HARC_AMD_SELECT_PIECE": "5000", "HARC_AMD_SELECT_LINES": "100"})
    assert r.returncode == 0, r.stdout[-3000:]
    assert (d / "x.sel.d.fastq").read_bytes() == want
    assert "[select] %d names, %d found, %d of %d records" % (k + 1, k, k, n) in r.stdout and "[select] not found: nobody" in r.stdout, r.stdout[-3000:]
    if kind == "packed":                                              # the archive of -V is checked whole, in front of the selection
        assert "[check] reads ok, order ok, ids ok, quality ok" in r.stdout and r.stdout.index("[check]") < r.stdout.index("[select]"), r.stdout[-3000:]
        assert _left(d, "x") == ["x.sel.d.fastq"]
        return                                                        # (-z goes through the same unchanged assembly: the other two kinds run it)
    r = _harc(["-d", str(d / "x.harc"), "-p", "-q", "-z", "-L", str(d / "names.txt")])
    assert r.returncode == 0, r.stdout[-3000:]
    gz = (d / "x.sel.d.fastq.gz").read_bytes()
    assert gzip.decompress(gz) == want and gz == harc_amd.bgzf_deflate_host(want)
    assert _left(d, "x") == ["x.sel.d.fastq", "x.sel.d.fastq.gz"]     # a selection never stands in for a full restore, and output/ is gone


@pytest.mark.parametrize("style", ["slash", "space", "none"])
def test_harc_selects_pairs_and_keeps_mates_together(style, root):
    d, (a, b) = _archive("pair_" + style, root)
    a_ids, b_ids = a.split(b"\n")[0:-1:4], b.split(b"\n")[0:-1:4]
    # names from file 1's ids, and for some pairs the second mate's id alone
    names = _list_of(a, 41) + b"".join(sc.key(l) + (b"/2" if style != "none" else b"") + b"\n" for l in b_ids[5::97])
    (d / "names.txt").write_bytes(names)
    fa, fb = sc.fastq_flags(a, names), sc.fastq_flags(b, names)
    both = bytes(x | y for x, y in zip(fa, fb))
    if style == "none":
        assert any(y and not x for x, y in zip(fa, fb)) and any(x and not y for x, y in zip(fa, fb))
    k = sum(both)
    assert 5 < k < 40
    r = _harc(["-d", str(d / "x.harc"), "-p", "-q", "-L", str(d / "names.txt")], {"HARC_AMD_SELECT_PIECE": "3000", "HARC_AMD_SELECT_LINES": "64"})
    assert r.returncode == 0, r.stdout[-3000:]
    assert (d / "x.sel.d.1.fastq").read_bytes() == sc.select_fastq(a, b"", also=both)
    assert (d / "x.sel.d.2.fastq").read_bytes() == sc.select_fastq(b, b"", also=both)
    assert "%d of 400 records" % k in r.stdout, r.stdout[-3000:]
    assert _left(d, "x") == ["x.sel.d.1.fastq", "x.sel.d.2.fastq"]
    # a list that names only the second mate of one pair selects that pair
    x = sc.key(b_ids[7])
    (d / "one.txt").write_bytes(x + (b"/2\n" if style != "none" else b"\n"))
    r = _harc(["-d", str(d / "x.harc"), "-p", "-q", "-L", str(d / "one.txt")])
    assert r.returncode == 0 and "1 names, 1 found, 1 of 400 records" in r.stdout, r.stdout[-3000:]
    assert (d / "x.sel.d.1.fastq").read_bytes() == b"".join(l + b"\n" for l in a.split(b"\n")[28:32])
    assert (d / "x.sel.d.2.fastq").read_bytes() == b"".join(l + b"\n" for l in b.split(b"\n")[28:32])


def test_harc_selects_in_stored_order_without_p(root):
    d, fq = _archive("stored", root)
    names = _list_of(fq, 29)
    (d / "names.txt").write_bytes(names)
    r = _harc(["-d", str(d / "x.harc"), "-q"])
    assert r.returncode == 0, r.stdout[-3000:]
    full = (d / "x.d.fastq").read_bytes()
    os.remove(d / "x.d.fastq")
    r = _harc(["-d", str(d / "x.harc"), "-q", "-L", str(d / "names.txt")])
    assert r.returncode == 0, r.stdout[-3000:]
    got = (d / "x.sel.d.fastq").read_bytes()
    assert got == sc.select_fastq(full, names)                        # a filter of what the full restore writes, in its order
    assert sorted(got.split(b"\n")[0:-1:4]) == sorted(sc.select_fastq(fq, names).split(b"\n")[0:-1:4])


def test_harc_a_list_that_matches_nothing_is_status_1_and_writes_nothing(root):
    d, fq = _archive("plain", root)
    before = _left(d, "x")
    (d / "nothing.txt").write_bytes(b"nobody\nSRR870667.0\nSRR870667.12000\n")
    for args in (["-p", "-q"], ["-p", "-q", "-z"]):
        r = _harc(["-d", str(d / "x.harc")] + args + ["-L", str(d / "nothing.txt")])
        assert r.returncode == 1 and "[select] no record of x carries one of the 3 names" in r.stdout, r.stdout[-3000:]
        assert _left(d, "x") == before
