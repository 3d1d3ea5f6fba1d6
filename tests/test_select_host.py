"""Selection by name on the host: harc_amd_name_key_host, harc_amd_select_flags_host and harc_amd_lines_gather_host -- the twins the kernels of select.hip are held
to -- against the plain-Python restatement of tests/select_cases.py on every case, the flags under HARC_AMD_SELECT_HASH_BITS 64, 8 and 1 (with a few bits different
names share a hash and a slot chain: the byte comparison and the probing decide), and the sizes the README quotes.  No GPU."""
import os
import re
from pathlib import Path

import pytest

import harc_amd
from tests import select_cases as sc

ROOT = Path(__file__).resolve().parents[1]
CASES = sc.cases()


@pytest.fixture
def hash_bits(monkeypatch):
    def set_bits(b):
        if b == 64:
            monkeypatch.delenv("HARC_AMD_SELECT_HASH_BITS", raising=False)
        else:
            monkeypatch.setenv("HARC_AMD_SELECT_HASH_BITS", str(b))
    return set_bits


def test_the_rule_of_the_issue_text():
    for line in (b"@r7/1 comment", b"r7/2", b"@r7", b"r7 x", b"r7\tx"):
        assert sc.key(line) == b"r7"
    assert sc.key(b"r70") == b"r70"
    assert sc.key(b"a/1/2") == b"a/1" and sc.key(b"a/1") == b"a" and sc.key(b"/1") == b"/1" and sc.key(b"ab/3") == b"ab/3"
    assert sc.key(b"@") == b"" and sc.key(b"") == b"" and sc.key(b"@ x") == b"" and sc.key(b"a\r") == b"a\r"


def test_name_key_host_equals_the_restatement_on_every_line():
    for line in sc.id_lines():
        assert harc_amd.name_key(line) == sc.key_span(line), line
        off, n = harc_amd.name_key(line)
        assert line[off:off + n] == sc.key(line), line


@pytest.mark.parametrize("bits", [64, 8, 1])
def test_select_flags_host_equals_the_restatement(hash_bits, bits):
    hash_bits(bits)
    for name in sorted(CASES):
        names, ids = CASES[name]
        got = harc_amd.select_flags_host(names, ids)
        assert got == (sc.flags(names, ids),) + sc.counts(names, ids), (name, bits)


def test_the_cases_cover_what_they_claim():
    names, ids = CASES["every third name"]
    f = sc.flags(names, ids)
    assert 0 < sum(f) < len(f)
    assert sum(sc.flags(*CASES["no matching name"])) == 0
    n, found = sc.counts(*CASES["duplicates, empty lines, comments, no final newline"])
    assert found < n and not CASES["duplicates, empty lines, comments, no final newline"][0].endswith(b"\n")
    assert sc.missing(*CASES["duplicates, empty lines, comments, no final newline"]) == [b"absent"]
    lens = {len(sc.key(l)) for l in sc.id_lines()}
    assert set(sc.NAME_LENGTHS) <= lens


def test_an_empty_list_and_an_empty_text():
    assert harc_amd.select_flags_host(b"", b"@a\n@b\n") == (b"\0\0", 0, 0)
    assert harc_amd.select_flags_host(b"a\n", b"") == (b"", 1, 0)
    assert harc_amd.select_flags_host(b"\n@\n \n", b"@\n\n") == (b"\0\0", 0, 0)


def test_lines_gather_host_equals_the_restatement():
    for name, (text, f, stride) in sorted(sc.gather_cases().items()):
        assert harc_amd.lines_gather_host(text, f, stride) == sc.gather(text, f, stride), name


def test_lines_gather_host_refuses_counts_that_do_not_fit():
    with pytest.raises(harc_amd.HarcAmdError, match="3 lines of 2 bytes are not the 5 bytes"):
        harc_amd.lines_gather_host(b"a\nb\nc", bytes(3), 2)
    with pytest.raises(harc_amd.HarcAmdError, match="holds 2 lines, the flags are those of 3"):
        harc_amd.lines_gather_host(b"a\nb\n", bytes(3), 0)


def test_select_fastq_keeps_whole_records_in_order():
    fq = b"@a/1 x\nAC\n+\nII\n@b\nGT\n+\nJJ\n@c\nTT\n+\nKK\n"
    assert sc.select_fastq(fq, b"c\na\n") == b"@a/1 x\nAC\n+\nII\n@c\nTT\n+\nKK\n"
    assert sc.select_fastq(fq, b"nobody\n") == b""
    assert sc.fastq_flags(fq, b"b\n") == bytes([0, 1, 0])


def test_the_sizes_the_readme_quotes():
    """the README's end-to-end figures are for 2 000 000 reads of 100 with ids of 13 bytes and a list of a hundredth of the names: the bytes written that it
    quotes for the full restore and for the selection are those of such files"""
    text = (ROOT / "README.md").read_text()
    sec = text[text.index("**`-L` and what it promises.**"):text.index("**`-P` and what it promises.**")]
    assert "2 000 000 reads of 100" in sec and "(20 000)" in sec
    record = 13 + 1 + 100 + 1 + 2 + 100 + 1
    quoted = [int(m.replace(" ", "")) for m in re.findall(r"(\d{1,3}(?: \d{3})+) bytes", sec)]
    assert 2_000_000 * record in quoted and 20_000 * record in quoted, quoted
    # the kernel figures are for lines of 76 bytes: floor(2^30 / 76) of them
    assert "76 bytes a line (14.1 M lines)" in sec and (1 << 30) // 76 == 14128181
