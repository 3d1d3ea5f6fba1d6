"""The line select of the range restore on the host (harc_amd/csrc/linesel.h): the twin the kernels are held to against bytes.split, and the refusals of the
packed side files' range calls that are decided before a device is touched -- a block prefix that leaves the file, a range beyond the header's line count."""
import pytest

from tests import id_cases
from tests import quality_cases as qc
from tests import range_cases as rc


@pytest.mark.parametrize("name", sorted(rc.texts()))
def test_the_host_twin_is_bytes_split(name):
    import harc_amd
    text = rc.texts()[name]
    for k in rc.ks(text):
        assert harc_amd.line_offset_host(text, k) == rc.line_offset(text, k), (name, k)
    nl = text.count(b"\n")
    assert harc_amd.line_offset_host(text, nl + 1)[1] == harc_amd.LINE_NONE == rc.NONE
    assert harc_amd.line_offset_host(text, 0) == (nl, 0)


def test_every_line_of_a_text_of_lines_of_every_short_length():
    import harc_amd
    text = rc.lines_of_lengths(list(range(0, 40)) + [0, 0, 0, 17, 0])
    lines = rc.lines_of(text)
    at = 0
    for k, line in enumerate(lines):
        assert harc_amd.line_offset_host(text, k) == (len(lines), at), k
        assert rc.slice_lines(text, k, 1) == text[at:at + len(line)] == line
        at += len(line)
    assert harc_amd.line_offset_host(text, len(lines)) == (len(lines), len(text))
    assert harc_amd.line_offset_host(text + b"open", len(lines)) == (len(lines), len(text))       # an open last line is no line, but it starts somewhere
    assert harc_amd.line_offset_host(text + b"open", len(lines) + 1) == (len(lines), rc.NONE)
    assert harc_amd.build_has("range")


def test_slice_lines_states_the_contract():
    text = b"a\n\nccc\ndd\n"
    assert rc.slice_lines(text, 0, 4) == text and rc.slice_lines(text, 1, 2) == b"\nccc\n" and rc.slice_lines(text, 3, 1) == b"dd\n"
    assert rc.slice_lines(text + b"open", 3, 5) == b"dd\n" and rc.slice_lines(b"", 0, 1) == b""
    fq = b"@a\nAC\n+\nHH\n@b\nGT\n+\nII\n"
    assert rc.slice_records(fq, 1, 1) == b"@b\nGT\n+\nII\n"


def _packed_quality():
    text = qc.markov(1500, 40, seed=3)
    import harc_amd
    return text, harc_amd.qpack_host(text, 40, 64)


def _packed_ids():
    text = id_cases.text(id_cases.ids(3000))
    import harc_amd
    return text, harc_amd.idpack_host(text, 512)


@pytest.mark.parametrize("kind", ["quality", "ids"])
def test_a_range_beyond_the_header_is_refused_naming_both(kind, tmp_path):
    import harc_amd
    text, packed = _packed_quality() if kind == "quality" else _packed_ids()
    n = text.count(b"\n")
    call = harc_amd.qunpack_range_files if kind == "quality" else harc_amd.idunpack_range_files
    f, out = tmp_path / "x.packed", tmp_path / "x.out"
    f.write_bytes(packed)
    for first, count, last in ((n, 1, n + 1), (n - 1, 2, n + 1), (0, n + 1, n + 1), (5 * n, 7, 5 * n + 7), (3, 0, 3)):
        with pytest.raises(harc_amd.HarcAmdError) as e:
            call(str(f), str(out), first, count)
        assert e.value.code == -1 and "lines %d .. %d are wanted" % (first + 1, last) in str(e.value) and "holds %d lines" % n in str(e.value), str(e.value)
        assert not out.exists()


@pytest.mark.parametrize("kind", ["quality", "ids"])
def test_a_prefix_that_leaves_the_file_is_refused_naming_the_block(kind, tmp_path):
    """the file is cut inside block 5: a range that needs block 5 or a later one is refused by the walk, before a device is asked for"""
    import harc_amd
    text, packed = _packed_quality() if kind == "quality" else _packed_ids()
    rb = 64 if kind == "quality" else 512
    call = harc_amd.qunpack_range_files if kind == "quality" else harc_amd.idunpack_range_files
    # where block 5 starts: the walk of the 4-byte prefixes, as the library does it
    at = 32
    for _ in range(5):
        at += 4 + int.from_bytes(packed[at:at + 4], "little")
    f, out = tmp_path / "x.packed", tmp_path / "x.out"
    f.write_bytes(packed[:at + 12])
    for first, count in ((5 * rb, 1), (5 * rb + 3, rb // 4), (4 * rb, rb + 1)):
        with pytest.raises(harc_amd.HarcAmdError) as e:
            call(str(f), str(out), first, count)
        assert e.value.code == -1 and "block 5 at byte %d leaves" % at in str(e.value), str(e.value)
        assert not out.exists()
    f.write_bytes(packed[:at + 2])                                 # not even the prefix of block 5 is whole
    with pytest.raises(harc_amd.HarcAmdError) as e:
        call(str(f), str(out), 5 * rb, 1)
    assert e.value.code == -1 and "block 5 at byte %d leaves" % at in str(e.value), str(e.value)
