"""The four file calls that carry the cut tail of an id text from piece to piece -- fastq_assemble, select_files, idmate_rule_files, idpack_files -- held to one
family of small texts (tests/line_walk_cases.py) in pieces that end on every newline, a byte behind every newline, inside a line that is longer than several
pieces, and nowhere.  The answer never depends on the piece.  An open last line counts as a line for fastq_assemble and select_files and is refused (EINVAL) by
idmate_rule_files and idpack_files.

idpack_files counts its piece in blocks of lines and never goes below 4 KiB of text: beside HARC_AMD_IDPACK_PIECE = the piece, every text is packed once in
blocks of 4 lines with a piece of 1 block, so that the text `wide` is cut inside a line at 4 KiB and calls of one block follow each other."""
import pytest

from tests import line_walk_cases as wc

pytestmark = pytest.mark.gpu
EINVAL = -1
TEXTS = wc.texts()
NAMES = sorted(TEXTS)


@pytest.fixture(autouse=True)
def _small_ring(monkeypatch):
    monkeypatch.setenv("HARC_AMD_FEED_SLICE", "256")


def _write(where, **texts):
    for k, v in texts.items():
        (where / k).write_bytes(v)
    return {k: str(where / k) for k in texts}


@pytest.mark.parametrize("name", NAMES)
def test_fastq_assemble_equals_the_join_whatever_the_piece(name, tmp_path, monkeypatch):
    import harc_amd
    ids, w = TEXTS[name]
    n = len(wc.lines(ids))
    dna, quality = wc.fixed(n, b"A"), wc.fixed(n, b"I")
    p = _write(tmp_path, i=ids, d=dna, q=quality)
    want = wc.join(ids, dna, quality)
    assert want.count(b"\n") == 4 * n
    for piece in wc.pieces(w):
        monkeypatch.setenv("HARC_AMD_FQOUT_PIECE", str(piece))
        out = tmp_path / ("o.%d" % piece)
        harc_amd.fastq_assemble(p["d"], p["i"], p["q"], str(out))
        assert out.read_bytes() == want, (name, piece)


@pytest.mark.parametrize("name", NAMES)
def test_select_files_equals_the_filter_by_name_whatever_the_piece(name, tmp_path, monkeypatch):
    import harc_amd
    ids, w = TEXTS[name]
    ls = wc.lines(ids)
    n = len(ls)
    dna, quality, names = wc.fixed(n, b"A"), wc.fixed(n, b"I"), wc.listed(ids)
    listed = set(wc.lines(names))
    flags = bytes(1 if wc.name(l) in listed else 0 for l in ls)
    p = _write(tmp_path, n=names, i=ids, d=dna, q=quality)
    outs = [str(tmp_path / x) for x in ("oi", "od", "oq")]
    if not n:                                                        # no read, no read length: the call refuses the job before it walks anything
        with pytest.raises(harc_amd.HarcAmdError) as e:
            harc_amd.select_files(p["n"], p["i"], p["d"], p["q"], *outs)
        assert e.value.code == EINVAL and not any((tmp_path / x).exists() for x in ("oi", "od", "oq")), str(e.value)
        return
    host_flags, distinct, found = harc_amd.select_flags_host(names, ids)
    assert host_flags == flags and (distinct, found) == (len(listed), len(listed) - 1)
    kept = b"".join(l for l, f in zip(ids.splitlines(True), flags) if f)              # with their newlines; an open last line as it is
    want = (kept, harc_amd.lines_gather_host(dna, flags, 7), harc_amd.lines_gather_host(quality, flags, 7))
    assert kept == harc_amd.lines_gather_host(ids, flags) and len(want[1]) == len(want[2]) == 7 * sum(flags)
    for piece in wc.pieces(w):
        monkeypatch.setenv("HARC_AMD_SELECT_PIECE", str(piece))
        st = harc_amd.select_files(p["n"], p["i"], p["d"], p["q"], *outs)
        assert st == (distinct, found, sum(flags), n, [b"nobody"]), (name, piece)
        assert tuple(open(x, "rb").read() for x in outs) == want, (name, piece)


@pytest.mark.parametrize("name", NAMES)
def test_idmate_rule_files_equals_the_host_rule_whatever_the_piece(name, tmp_path, monkeypatch):
    import harc_amd
    ids, w = TEXTS[name]
    for k, mate in enumerate(wc.mates(ids)):
        p = _write(tmp_path, a=ids, b=mate)
        for piece in wc.pieces(w):
            monkeypatch.setenv("HARC_AMD_IDMATE_PIECE", str(piece))
            for x, y in ((ids, mate), (mate, ids), (ids, ids)):
                px, py = (p["a"] if x is ids else p["b"]), (p["a"] if y is ids else p["b"])
                if name.endswith("_open") and (x is ids or y is ids):
                    with pytest.raises(harc_amd.HarcAmdError) as e:
                        harc_amd.idmate_rule_files(px, py)
                    assert e.value.code == EINVAL and "no newline" in str(e.value), (name, k, piece, str(e.value))
                else:
                    assert harc_amd.idmate_rule_files(px, py) == harc_amd.idmate_rule_host(x, y)[:2], (name, k, piece)


@pytest.mark.parametrize("name", NAMES)
def test_idpack_files_writes_the_host_coder_s_bytes_and_idunpack_files_the_text(name, tmp_path, monkeypatch):
    import harc_amd
    ids, w = TEXTS[name]
    p = _write(tmp_path, i=ids)
    monkeypatch.setenv("HARC_AMD_IDPACK_BLOCK", "4")
    for piece in [1] + wc.pieces(w):
        monkeypatch.setenv("HARC_AMD_IDPACK_PIECE", str(piece))
        packed, back = tmp_path / ("p.%d" % piece), tmp_path / ("b.%d" % piece)
        if name.endswith("_open"):
            with pytest.raises(harc_amd.HarcAmdError) as e:
                harc_amd.idpack_files(p["i"], str(packed))
            assert e.value.code == EINVAL and "newline" in str(e.value) and not packed.exists(), (name, piece, str(e.value))
            continue
        harc_amd.idpack_files(p["i"], str(packed))
        assert packed.read_bytes() == harc_amd.idpack_host(ids, 4), (name, piece)
        harc_amd.idunpack_files(str(packed), str(back))
        assert back.read_bytes() == ids, (name, piece)
